/*
 * gr4pm_hip.h -- C ABI of the MI355X-native gr4-packet-modem RX hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  The
 * gr::Block<T> wrappers in gr4-packet-modem_amd/host/ (and the ctypes binding used by the
 * tests) call exactly these entry points.  Each entry point cites the reference interface
 * it replaces; paths are relative to
 *   /root/reference/blocks/include/gnuradio-4.0/packet-modem/
 *
 * Conventions
 *  - Sample pointers (`in`, `out`) are DEVICE pointers (HBM resident) unless a function
 *    says otherwise; complex samples are interleaved float32 pairs == std::complex<float>.
 *  - Tag arrays, message arrays, settings and counters are HOST pointers.
 *  - Tags are passed with explicit item indices relative to in[0] of the call (the GR4
 *    runtime presents a tag only at the head of a chunk; the wrapper passes index 0).
 *  - One handle == one HIP stream == single-threaded use, like one gr::Block instance.
 *  - No exceptions cross the ABI.  Negative status == what the reference block throws as
 *    gr::exception; positive status == gr::work::Status other than OK.
 *  - Batched handles (n_channels > 1) process independent channels laid out as
 *    [channel][stride] in one launch; every channel has its own state.
 */
#ifndef GR4PM_HIP_H
#define GR4PM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { float re, im; } gr4pm_c64;

typedef enum {
    GR4PM_OK = 0,
    GR4PM_INSUFFICIENT_INPUT_ITEMS = 1,  /* gr::work::Status::INSUFFICIENT_INPUT_ITEMS */
    GR4PM_INSUFFICIENT_OUTPUT_ITEMS = 2, /* gr::work::Status::INSUFFICIENT_OUTPUT_ITEMS */
    GR4PM_ERR_INVALID = -1,              /* invalid settings (reference: throw gr::exception) */
    GR4PM_ERR_UNSUPPORTED = -2,          /* valid in the reference, not built here yet */
    GR4PM_ERR_HIP = -3,                  /* HIP runtime failure, see gr4pm_last_error() */
    GR4PM_ERR_NOMEM = -4,
    GR4PM_ERR_OVERFLOW = -5,             /* a caller-provided tag/record array was too small */
    GR4PM_ERR_NO_DEVICE = -6,            /* no HIP device: the product has no CPU fallback */
    GR4PM_ERR_INTERNAL = -7              /* a C++ exception other than std::bad_alloc (which is GR4PM_ERR_NOMEM) was caught
                                            at the ABI or in one of the handle's threads: gr4pm_last_error() has what() */
} gr4pm_status;

/* Human readable text of the last failure on the calling thread. */
const char* gr4pm_last_error(void);
/* Library version / build info; also proves the HIP code objects are loaded. */
const char* gr4pm_version(void);
/* Number of visible HIP devices (0 when none; does not create a context). */
int gr4pm_device_count(void);
/* For native callers that chain several handles on ONE HIP stream without reading anything back in
 * between: while on (per calling thread), the process() calls that return nothing device-produced
 * to the host (symbol filter, wipe-off, Costas loop, PayloadMetadataInsert, SyncwordRemove, LLR
 * decoder, scrambler, HeaderPayloadSplit, slicer / packer) do not wait for their stream; the
 * caller synchronises the stream before it reads their outputs, hands them to another stream, or
 * calls the same handle again. */
void gr4pm_set_deferred_sync(int on);

/* The `syncword_*` tag set published by SyncwordDetection (syncword_detection.hpp:106-114)
 * and consumed downstream (symbol_filter.hpp:130-156, coarse_frequency_correction.hpp:78-80,
 * costas_loop.hpp:101-106, syncword_wipeoff.hpp:53-62). */
typedef struct {
    uint64_t index;    /* item index the tag is attached to */
    float amplitude;   /* "syncword_amplitude" */
    float phase;       /* "syncword_phase" */
    double freq;       /* "syncword_freq" (double in the reference) */
    int32_t freq_bin;  /* "syncword_freq_bin" */
    float noise_power; /* "syncword_noise_power" */
    float esn0_db;     /* "syncword_esn0_db" */
    float time_est;    /* "syncword_time_est" */
    int32_t flags;     /* GR4PM_TAG_* */
    int32_t user;      /* the caller's own cookie: never read by the library, copied with the tag by every block that
                          re-emits it (SymbolFilter's re-timed tags, :218-228) -- a binding keeps the full property map
                          of a tag under this handle; SyncwordDetection writes 0.  (Round 6: the GR4 wrapper used to
                          carry its handle in freq_bin; the field takes the struct's former tail padding, size 48.) */
} gr4pm_tag;
#if defined(__cplusplus)
static_assert(sizeof(gr4pm_tag) == 48, "gr4pm_tag is 48 bytes (tests and bindings mirror it)");
#endif
#define GR4PM_TAG_SYNCWORD 1 /* carries the syncword_* keys */
#define GR4PM_TAG_OTHER 2    /* carries other (opaque, wrapper-held) keys */

/* ------------------------------------------------------------------------------------
 * SyncwordDetection -- syncword_detection.hpp:32-357
 *   settings  :133-141      start() :143-202      processBulk() :204-356
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_syncword_detection gr4pm_syncword_detection;
typedef struct {
    size_t fft_size;           /* :133, default 2048 (tuned one-wave path); other powers of two
                                  256..8192 run the generic workgroup-per-block path */
    size_t samples_per_symbol; /* :134 */
    const float* rrc_taps;     /* :135 host */
    size_t n_rrc_taps;
    const uint8_t* syncword;   /* :136 host */
    size_t n_syncword;
    const gr4pm_c64* constellation; /* :137 host */
    size_t n_constellation;
    int min_freq_bin;          /* :138 */
    int max_freq_bin;          /* :139 */
    uint64_t time_threshold;   /* :140 */
    float power_threshold;     /* :141 */
    size_t n_channels;         /* independent channels per call (>= 1) */
    size_t max_items;          /* largest n_in per channel per call (workspace sizing) */
    void* stream;              /* hipStream_t, NULL = default stream */
} gr4pm_syncword_detection_params;

gr4pm_status gr4pm_syncword_detection_create(const gr4pm_syncword_detection_params* params,
                                             gr4pm_syncword_detection** out);
void gr4pm_syncword_detection_destroy(gr4pm_syncword_detection* h);
/* == start(): clears _best/_best_idx/_items_consumed/_history (:191-199) */
gr4pm_status gr4pm_syncword_detection_reset(gr4pm_syncword_detection* h);
/* public state the reference exposes and its tests read (test/qa_syncword_detection.cpp:101-133) */
size_t gr4pm_syncword_detection_syncword_samples_size(const gr4pm_syncword_detection* h);
float gr4pm_syncword_detection_self_corr(const gr4pm_syncword_detection* h);
uint64_t gr4pm_syncword_detection_items_consumed(const gr4pm_syncword_detection* h);
/* Diagnostics of the last process() call (no reference counterpart): how many candidates the scan visited in the channel
 * (the items whose history the reference tests, :268-279) and how many of those were tested by the separate pass over
 * the powers instead of on the candidate kernel's registers (all of them for a time_threshold other than 768). */
void gr4pm_syncword_detection_scan_counts(const gr4pm_syncword_detection* h, size_t channel, uint64_t* visited,
                                          uint64_t* tested_from_memory);
/* == processBulk().  in: [n_channels][in_stride] items, n_in valid per channel.
 * out: [n_channels][out_stride] or NULL (skip the delayed pass-through copy when the
 * consumer reads the input ring itself).  *n_done = items consumed == published per channel
 * (whole strides only, :238,346-350).  tags: host [n_channels][tags_cap], n_tags: host
 * [n_channels]; tag.index is relative to out[0] of this call.  Returns
 * GR4PM_INSUFFICIENT_INPUT_ITEMS when n_in < fft_size (:215-227). */
gr4pm_status gr4pm_syncword_detection_process(gr4pm_syncword_detection* h, const gr4pm_c64* in,
                                              size_t in_stride, size_t n_in, gr4pm_c64* out,
                                              size_t out_stride, size_t* n_done, gr4pm_tag* tags,
                                              size_t tags_cap, size_t* n_tags);
/* Optional look-ahead for callers that own a device ring (no reference counterpart: the
 * reference's scheduler overlaps blocks across worker threads instead).  _announce names the
 * input of a future call: the one after the next process() and after the calls already
 * announced (at most GR4PM_SD_LOOKAHEAD = 2 calls ahead are kept; further announcements are
 * ignored).  The next process() then also launches, on two more streams, everything of the
 * announced calls that does not depend on the scan state of the calls before them (z carry,
 * correlator, candidate bitmap, tile / group tables), where it overlaps this call's scan, tag
 * kernels and read-back; the later process(in, in_stride, n_in) with exactly the announced
 * arguments finds that work done.  The items must not change between the announcement and
 * their call, and whatever produces them must have been queued on the handle's stream (or have
 * finished) when they are announced: the look-ahead streams wait for an event recorded on the
 * handle's stream at announcement time before they read an announced buffer.  A call with other arguments drops the look-ahead and recomputes; results are
 * identical either way.  _hint_next is the one-call form: it replaces every announcement not
 * yet launched (in_next == NULL: just clears them). */
#define GR4PM_SD_LOOKAHEAD 2
gr4pm_status gr4pm_syncword_detection_announce(gr4pm_syncword_detection* h, const gr4pm_c64* in,
                                               size_t in_stride, size_t n_in);
gr4pm_status gr4pm_syncword_detection_hint_next(gr4pm_syncword_detection* h,
                                                const gr4pm_c64* in_next, size_t in_stride,
                                                size_t n_next);
/* debug / measurement: copies the per-sample best-bin correlation power of the last call
 * (device [n_channels][n_done] floats, items_consumed-relative) into `zpow` (device). */
gr4pm_status gr4pm_syncword_detection_last_zpow(gr4pm_syncword_detection* h, float* zpow,
                                                size_t stride);
/* measurement hook: runs ONLY the overlap-save correlator kernel on [n_channels][in_stride]
 * input (no detector, no copy); used by bench.py to time the dominant kernel in isolation. */
gr4pm_status gr4pm_syncword_detection_correlate_only(gr4pm_syncword_detection* h,
                                                     const gr4pm_c64* in, size_t in_stride,
                                                     size_t n_in);

/* ------------------------------------------------------------------------------------
 * SyncwordDetectionFilter<T = c64> -- syncword_detection_filter.hpp:10-211
 * One call == one processBulk() (:54-210) with the messages pending on the two async
 * ports.  Samples are copied device-to-device; the tag gate runs on the host.
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_syncword_detection_filter gr4pm_syncword_detection_filter;
typedef struct {
    size_t samples_per_symbol; /* :44 */
    size_t syncword_size;      /* :45 */
    size_t header_size;        /* :46 */
    void* stream;
} gr4pm_syncword_detection_filter_params;
typedef struct {
    uint64_t packet_length; /* "packet_length" of a parsed_header message */
    int32_t invalid_header; /* 1: message carries "invalid_header"; 2 (headers_per_tag modes only):
                               no message yet, see ..._gate_resolve / ..._insert_resolve */
} gr4pm_header_msg;
gr4pm_status gr4pm_syncword_detection_filter_create(
    const gr4pm_syncword_detection_filter_params* params, gr4pm_syncword_detection_filter** out);
void gr4pm_syncword_detection_filter_destroy(gr4pm_syncword_detection_filter* h);
gr4pm_status gr4pm_syncword_detection_filter_reset(gr4pm_syncword_detection_filter* h);
/* head_tag_flags: GR4PM_TAG_* of the tag at in[0], 0 if none.  *tag_out_flags: which key
 * classes are published at out[0] (:82-104). */
gr4pm_status gr4pm_syncword_detection_filter_process(
    gr4pm_syncword_detection_filter* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out,
    size_t out_cap, int head_tag_flags, const gr4pm_header_msg* headers, size_t n_headers,
    size_t n_ignored, size_t* consumed, size_t* headers_consumed, size_t* ignored_consumed,
    int* tag_out_flags);

/* Tag gate only (no sample copy), for device-resident chains where the filter's copy is folded
 * into its neighbours: replays :75-105,134-185 over a sorted list of syncword tag indices
 * (absolute item indices of the stream).  headers_per_tag == 0: headers[k] is the parsed_header
 * message that answers the k-th ACCEPTED tag; != 0: headers[i] answers tag i if it is accepted
 * (n_headers == n_tags).  The reference blocks the stream until that message arrives
 * (:164-185), so the outcome does not depend on message timing.  accepted[i] = 1 when tag i
 * passes.  State (in-packet span) carries across calls.  *headers_used = messages consumed. */
gr4pm_status gr4pm_syncword_detection_filter_gate(gr4pm_syncword_detection_filter* h,
                                                  const uint64_t* tag_index, size_t n_tags,
                                                  const gr4pm_header_msg* headers, size_t n_headers,
                                                  int headers_per_tag, uint8_t* accepted,
                                                  size_t* headers_used);
/* headers_per_tag mode, header decoded on the device: the message of the LAST accepted tag of a
 * call may not exist yet when its header symbols continue in the next batch.  Mark it
 * invalid_header = 2 ("pending") and deliver it with this call before the next gate(). */
gr4pm_status gr4pm_syncword_detection_filter_gate_resolve(gr4pm_syncword_detection_filter* h,
                                                          const gr4pm_header_msg* msg);

/* ------------------------------------------------------------------------------------
 * CoarseFrequencyCorrection<float> -- coarse_frequency_correction.hpp:20-99
 * Rotator<float>                   -- rotator.hpp:20-65
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_rotator gr4pm_rotator;
typedef struct {
    int mode;          /* 0: Rotator (phase_incr), 1: CoarseFrequencyCorrection (delay) */
    float phase_incr;  /* rotator.hpp:42 */
    size_t delay;      /* coarse_frequency_correction.hpp:43 */
    size_t n_channels; /* independent channels, state per channel */
    void* stream;
} gr4pm_rotator_params;
gr4pm_status gr4pm_rotator_create(const gr4pm_rotator_params* params, gr4pm_rotator** out);
void gr4pm_rotator_destroy(gr4pm_rotator* h);
gr4pm_status gr4pm_rotator_reset(gr4pm_rotator* h);
/* Rotator: tags ignored.  CFC: every tag with GR4PM_TAG_SYNCWORD re-loads the frequency
 * `delay` items later (:50-59,76-96).  tags: host, sorted by index, channel 0 only when
 * n_channels == 1; for batches use tag_channel[] to address channels. */
gr4pm_status gr4pm_rotator_process(gr4pm_rotator* h, const gr4pm_c64* in, size_t stride,
                                   size_t n, gr4pm_c64* out, const gr4pm_tag* tags,
                                   const uint32_t* tag_channel, size_t n_tags);

/* ------------------------------------------------------------------------------------
 * CostasLoop<float,float> -- costas_loop.hpp:15-149
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_costas_loop gr4pm_costas_loop;
typedef struct {
    double loop_bandwidth; /* :48 */
    int constellation;     /* constellation.hpp: 0 PILOT, 1 BPSK, 2 QPSK */
    size_t n_channels;
    void* stream;
} gr4pm_costas_loop_params;
gr4pm_status gr4pm_costas_loop_create(const gr4pm_costas_loop_params* params,
                                      gr4pm_costas_loop** out);
void gr4pm_costas_loop_destroy(gr4pm_costas_loop* h);
gr4pm_status gr4pm_costas_loop_reset(gr4pm_costas_loop* h);
void gr4pm_costas_loop_coeffs(const gr4pm_costas_loop* h, float* k1, float* k2);
/* settingsChanged() (:52-88): new constellation / loop bandwidth from tags or messages */
gr4pm_status gr4pm_costas_loop_set(gr4pm_costas_loop* h, double loop_bandwidth,
                                   int constellation);
/* same results either way.  on = 1: the kernel of _process / _process_ragged keeps to 62 VGPRs, on = 2: to 32 VGPRs
 * (what a SIMD has left beside two waves of the syncword correlator: the PLL's waves then run BESIDE a correlator
 * workgroup instead of keeping a compute unit from it) at the price of being slower by itself -- for callers that run
 * it next to a SyncwordDetection: the pipelined gr4pm_packet_receiver asks for 2.  Form 2 is only taken for calls of
 * 2^25 symbols and more: a PLL wave lives for one packet's chain however small the call, so below that the receiver
 * waits for the kernel's own speed (gr4pm_multichannel_receiver keeps form 0: measured) */
gr4pm_status gr4pm_costas_loop_set_small_footprint(gr4pm_costas_loop* h, int on);
gr4pm_status gr4pm_costas_loop_process(gr4pm_costas_loop* h, const gr4pm_c64* in, size_t stride,
                                       size_t n, gr4pm_c64* out, const gr4pm_tag* tags,
                                       const uint32_t* tag_channel, size_t n_tags);
/* the same with a different item count per channel (n_per_channel: host [n_channels]) */
gr4pm_status gr4pm_costas_loop_process_ragged(gr4pm_costas_loop* h, const gr4pm_c64* in, size_t stride,
                                              const size_t* n_per_channel, gr4pm_c64* out,
                                              const gr4pm_tag* tags, const uint32_t* tag_channel,
                                              size_t n_tags);

/* ------------------------------------------------------------------------------------
 * SyncwordWipeoff<c64,float> -- syncword_wipeoff.hpp:12-91
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_syncword_wipeoff gr4pm_syncword_wipeoff;
typedef struct {
    const float* syncword; /* :37 host */
    size_t n_syncword;
    void* stream;
} gr4pm_syncword_wipeoff_params;
gr4pm_status gr4pm_syncword_wipeoff_create(const gr4pm_syncword_wipeoff_params* params,
                                           gr4pm_syncword_wipeoff** out);
void gr4pm_syncword_wipeoff_destroy(gr4pm_syncword_wipeoff* h);
gr4pm_status gr4pm_syncword_wipeoff_reset(gr4pm_syncword_wipeoff* h);
/* `out` may be `in` (in place: only the syncword items are touched, no copy) */
gr4pm_status gr4pm_syncword_wipeoff_process(gr4pm_syncword_wipeoff* h, const gr4pm_c64* in,
                                            size_t n, gr4pm_c64* out, const gr4pm_tag* tags,
                                            size_t n_tags);
/* many channels, in place, one launch (per channel SyncwordWipeoff::processBulk, syncword_wipeoff.hpp:38-90):
 * h[c] is channel c's block (one syncword for all), its items are
 * buf[c * stride .. c * stride + n[c]), its tags tags[c][0 .. n_tags[c]).  Runs on h[0]'s stream. */
gr4pm_status gr4pm_syncword_wipeoff_process_channels(gr4pm_syncword_wipeoff* const* h, size_t n_channels,
                                                     gr4pm_c64* buf, size_t stride, const size_t* n,
                                                     const gr4pm_tag* const* tags, const size_t* n_tags);

/* ------------------------------------------------------------------------------------
 * InterpolatingFirFilter<TIn,TOut,float> -- interpolating_fir_filter.hpp:14-103
 *   item_kind: 0 = std::complex<float>, 1 = float
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_interp_fir gr4pm_interp_fir;
typedef struct {
    size_t interpolation; /* :39 */
    const float* taps;    /* :40 host */
    size_t n_taps;
    int item_kind;
    void* stream;
} gr4pm_interp_fir_params;
gr4pm_status gr4pm_interp_fir_create(const gr4pm_interp_fir_params* params,
                                     gr4pm_interp_fir** out);
void gr4pm_interp_fir_destroy(gr4pm_interp_fir* h);
gr4pm_status gr4pm_interp_fir_reset(gr4pm_interp_fir* h);
/* consumes n_in items, produces n_in * interpolation items (:91-99) */
gr4pm_status gr4pm_interp_fir_process(gr4pm_interp_fir* h, const void* in, size_t n_in,
                                      void* out);

/* ------------------------------------------------------------------------------------
 * SymbolFilter<TIn,TOut,float> -- symbol_filter.hpp:13-253
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_symbol_filter gr4pm_symbol_filter;
typedef struct {
    size_t samples_per_symbol; /* :55 */
    const float* taps;         /* :56 host, prototype PFB taps */
    size_t n_taps;
    size_t num_arms;           /* :58 */
    size_t delay;              /* :59 */
    int item_kind;             /* 0 complex, 1 float */
    void* stream;
} gr4pm_symbol_filter_params;
gr4pm_status gr4pm_symbol_filter_create(const gr4pm_symbol_filter_params* params,
                                        gr4pm_symbol_filter** out);
void gr4pm_symbol_filter_destroy(gr4pm_symbol_filter* h);
gr4pm_status gr4pm_symbol_filter_reset(gr4pm_symbol_filter* h);
/* tags_in: host, sorted, indices relative to in[0]; tags_out: host, indices relative to
 * out[0] (re-timed to symbols, :204-228; syncword_phase adjusted when time_est < 0,
 * :148-156).  Stops when out_cap symbols were produced (:208). */
gr4pm_status gr4pm_symbol_filter_process(gr4pm_symbol_filter* h, const void* in, size_t n_in,
                                         void* out, size_t out_cap, const gr4pm_tag* tags_in,
                                         size_t n_tags_in, gr4pm_tag* tags_out, size_t tags_cap,
                                         size_t* n_tags_out, size_t* consumed, size_t* produced);

/* Fused CoarseFrequencyCorrection -> SymbolFilter (packet_receiver.hpp:221-224 connects them
 * back to back): same results and same state updates as gr4pm_rotator_process (mode 1) followed
 * by gr4pm_symbol_filter_process with the same tags, but the rotated stream is never written
 * to memory.  Both handles must be single-channel / complex and share one stream; out_cap must
 * cover all n_in items (n_in / samples_per_symbol + n_tags_in + 2). */
gr4pm_status gr4pm_cfc_symbol_filter_process(gr4pm_rotator* cfc, gr4pm_symbol_filter* sf,
                                             const gr4pm_c64* in, size_t n_in, gr4pm_c64* out,
                                             size_t out_cap, const gr4pm_tag* tags_in, size_t n_tags_in,
                                             gr4pm_tag* tags_out, size_t tags_cap, size_t* n_tags_out,
                                             size_t* consumed, size_t* produced);
/* The same call in two halves, for callers that pipeline them (the native PacketReceiver runs
 * them as two stages): _plan replays the CFC's tag handling and computes the phasor checkpoints
 * of the call on the CFC's stream (the serial part), _run is the filter itself on the
 * SymbolFilter's stream.  The caller orders them (a _run after its _plan has completed; plans
 * and runs each in stream order).  GR4PM_CFC_PLANS plans exist (a ring): a plan stays valid until
 * GR4PM_CFC_PLANS - 1 further plans have been made, so that many calls may sit between the two
 * halves.  `plan` is the value _plan returned.
 * Round 6: where chains are long (>= 2^17 items between two syncword_freq events) and the process has at least eight
 * hardware queues (GPU_MAX_HW_QUEUES), _plan leaves the chains running on streams of the CFC handle's own when it
 * returns -- those of consecutive plans side by side -- and _run makes the SymbolFilter's stream wait for them
 * (events); the caller's ordering rule is unchanged, what it gains is that the stage which makes the plans does not
 * wait for a chain.  GR4PM_ROT_SERIAL=1 (read when the handle is created): never. */
#define GR4PM_CFC_PLANS 12
gr4pm_status gr4pm_cfc_symbol_filter_plan(gr4pm_rotator* cfc, size_t n_in, const gr4pm_tag* tags_in,
                                          size_t n_tags_in, int* plan);
/* many channels: ONE CoarseFrequencyCorrection handle with n_channels channels plans all of them
 * in one launch (tags of all channels, tag_channel[i] = channel of tags_in[i], indices relative
 * to the channel's first item); every channel's own SymbolFilter then runs with
 * _run_channel(plan, channel, ...), `in` pointing at that channel's items */
gr4pm_status gr4pm_cfc_symbol_filter_plan_channels(gr4pm_rotator* cfc, size_t n_in, const gr4pm_tag* tags_in,
                                                   const uint32_t* tag_channel, size_t n_tags_in, int* plan);
gr4pm_status gr4pm_cfc_symbol_filter_run_channel(gr4pm_rotator* cfc, int plan, size_t channel,
                                                 gr4pm_symbol_filter* sf, const gr4pm_c64* in, size_t n_in,
                                                 gr4pm_c64* out, size_t out_cap, const gr4pm_tag* tags_in,
                                                 size_t n_tags_in, gr4pm_tag* tags_out, size_t tags_cap,
                                                 size_t* n_tags_out, size_t* consumed, size_t* produced);
/* ... or ALL channels in ONE launch of the filter kernel (64 channels of 2^22 items are 64 small launches
 * otherwise; per channel it is SymbolFilter::processBulk, symbol_filter.hpp:112-252, fed by
 * CoarseFrequencyCorrection::processBulk, coarse_frequency_correction.hpp:67-98): sf[c] is channel c's SymbolFilter (one design for all; its tag-driven state is replayed on the
 * host exactly as by _run_channel), in: [n_channels][in_stride], out: [n_channels][out_stride] (out_stride >=
 * n_in / samples_per_symbol + tags + 2), tags_in[c] / n_tags_in[c] and tags_out[c] (tags_cap each) /
 * n_tags_out[c] / produced[c] per channel.  Runs on sf[0]'s stream.
 * Two-piece input (n_head > 0): the first n_head items of channel c's call are head[c * head_stride + i], item
 * i >= n_head is in[c * in_stride + i - n_head] -- SyncwordDetection's delayed stream read in place: the last
 * 2 * time_threshold + 1 items of the batch before, then this batch's own input (no delayed copy, 16 B/sample). */
gr4pm_status gr4pm_cfc_symbol_filter_run_channels(gr4pm_rotator* cfc, int plan, gr4pm_symbol_filter* const* sf,
                                                  size_t n_channels, const gr4pm_c64* in, size_t in_stride,
                                                  size_t n_in, gr4pm_c64* out, size_t out_stride,
                                                  const gr4pm_tag* const* tags_in, const size_t* n_tags_in,
                                                  gr4pm_tag* const* tags_out, size_t tags_cap, size_t* n_tags_out,
                                                  size_t* produced, const gr4pm_c64* head, size_t head_stride,
                                                  size_t n_head);
gr4pm_status gr4pm_cfc_symbol_filter_run(gr4pm_rotator* cfc, int plan, gr4pm_symbol_filter* sf,
                                         const gr4pm_c64* in, size_t n_in, gr4pm_c64* out,
                                         size_t out_cap, const gr4pm_tag* tags_in, size_t n_tags_in,
                                         gr4pm_tag* tags_out, size_t tags_cap, size_t* n_tags_out,
                                         size_t* consumed, size_t* produced);

/* ------------------------------------------------------------------------------------
 * PfbArbResampler<c64,c64,float,TRate> -- pfb_arb_resampler.hpp:23-183
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_pfb_arb_resampler gr4pm_pfb_arb_resampler;
typedef struct {
    double rate;        /* :63 */
    int rate_is_double; /* TRate: 0 float (default), 1 double */
    const float* taps;  /* :64 host; NULL = the built-in default prototype */
    size_t n_taps;
    size_t filter_size; /* :65 */
    void* stream;
} gr4pm_pfb_arb_resampler_params;
gr4pm_status gr4pm_pfb_arb_resampler_create(const gr4pm_pfb_arb_resampler_params* params,
                                            gr4pm_pfb_arb_resampler** out);
void gr4pm_pfb_arb_resampler_destroy(gr4pm_pfb_arb_resampler* h);
gr4pm_status gr4pm_pfb_arb_resampler_reset(gr4pm_pfb_arb_resampler* h);
gr4pm_status gr4pm_pfb_arb_resampler_process(gr4pm_pfb_arb_resampler* h, const gr4pm_c64* in,
                                             size_t n_in, gr4pm_c64* out, size_t out_cap,
                                             size_t* consumed, size_t* produced);

/* ====================================================================================
 * Symbol-rate control blocks behind SyncwordWipeoff: the immediate
 * consumers of the path's tags, closing the chain to soft bits on the device.
 * ================================================================================== */

/* Tags of this part of the chain (payload_metadata_insert.hpp:44-51).  Keys that name a
 * setting of a downstream block ("constellation", "loop_bandwidth") change that setting from
 * the tagged item on, like the reference's tag-driven settings. */
typedef struct {
    uint64_t index;           /* item index the tag is attached to */
    int32_t kind;             /* GR4PM_PKT_* */
    int32_t constellation;    /* "constellation": 0 PILOT, 1 BPSK, 2 QPSK; < 0: key absent */
    double loop_bandwidth;    /* "loop_bandwidth"; < 0: key absent */
    uint64_t packet_length;   /* GR4PM_PKT_PAYLOAD: "packet_length" of the parsed header */
    uint64_t payload_symbols; /* GR4PM_PKT_PAYLOAD: "payload_symbols" */
    uint64_t payload_bits;    /* GR4PM_PKT_PAYLOAD: "payload_bits" */
    gr4pm_tag syncword;       /* GR4PM_PKT_SYNCWORD: the syncword_* keys travelling along */
} gr4pm_packet_tag;
#define GR4PM_PKT_SYNCWORD 1     /* start of the (wiped-off) syncword, :104-112 */
#define GR4PM_PKT_HEADER_START 2 /* "header_start", :186-194 */
#define GR4PM_PKT_PAYLOAD 3      /* parsed header + payload sizes, :222-234 */

/* ------------------------------------------------------------------------------------
 * PayloadMetadataInsert<c64> -- payload_metadata_insert.hpp:12-324
 * One call == the processBulk() calls (:77-307) the runtime would make over n_in items, cut at
 * the syncword tags, with `headers` = the parsed_header messages pending, oldest first.  The
 * packet symbols are gathered device-to-device; everything between packets is dropped.
 * Where the reference returns to wait for a header (:243-247) the call stops: *consumed < n_in,
 * and the caller presents the rest again when the message is there.
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_payload_metadata_insert gr4pm_payload_metadata_insert;
typedef struct {
    size_t syncword_size;                  /* :60 */
    size_t header_size;                    /* :61 */
    double syncword_costas_loop_bandwidth; /* :62 */
    double header_costas_loop_bandwidth;   /* :63 */
    double payload_costas_loop_bandwidth;  /* :64 */
    void* stream;
} gr4pm_payload_metadata_insert_params;
gr4pm_status gr4pm_payload_metadata_insert_create(const gr4pm_payload_metadata_insert_params* params,
                                                  gr4pm_payload_metadata_insert** out);
void gr4pm_payload_metadata_insert_destroy(gr4pm_payload_metadata_insert* h);
gr4pm_status gr4pm_payload_metadata_insert_reset(gr4pm_payload_metadata_insert* h); /* start(), :71-75 */
/* tags_in: host, sorted, index relative to in[0]; only GR4PM_TAG_SYNCWORD tags matter.
 * headers_per_tag == 0: `headers` is the message queue, oldest first, one message per packet the
 * block opens.  != 0 (n_headers == n_tags_in): headers[i] answers tags_in[i] if that syncword
 * opens a packet, for callers that know every detection's header up front (same convention as
 * gr4pm_syncword_detection_filter_gate); the message of a packet still open at the end of the
 * call is kept.  tags_out: host, index relative to out[0].  *headers_used = messages consumed.
 * *ignored_syncwords: syncwords seen inside a packet (:126-147, the ignored_syncword messages). */
gr4pm_status gr4pm_payload_metadata_insert_process(
    gr4pm_payload_metadata_insert* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_cap,
    const gr4pm_tag* tags_in, size_t n_tags_in, const gr4pm_header_msg* headers, size_t n_headers,
    int headers_per_tag, gr4pm_packet_tag* tags_out, size_t tags_cap, size_t* n_tags_out, size_t* consumed,
    size_t* produced, size_t* headers_used, size_t* ignored_syncwords);

/* headers_per_tag mode: the message of a packet that was opened with a pending header
 * (invalid_header = 2) in an earlier call, delivered before the call that reaches its payload. */
gr4pm_status gr4pm_payload_metadata_insert_resolve(gr4pm_payload_metadata_insert* h,
                                                   const gr4pm_header_msg* msg);

/* CostasLoop fed by PayloadMetadataInsert (packet_receiver.hpp wiring): "constellation" and
 * "loop_bandwidth" keys re-run settingsChanged() (costas_loop.hpp:52-88) from the tagged item
 * on, GR4PM_PKT_SYNCWORD tags with the syncword_* keys set the phase (:101-106).  The new
 * settings stay in the handle.  Single channel. */
gr4pm_status gr4pm_costas_loop_process_packets(gr4pm_costas_loop* h, const gr4pm_c64* in, size_t n,
                                               gr4pm_c64* out, const gr4pm_packet_tag* tags,
                                               size_t n_tags);

/* ------------------------------------------------------------------------------------
 * SyncwordRemove<c64> -- syncword_remove.hpp:11-112
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_syncword_remove gr4pm_syncword_remove;
typedef struct {
    size_t syncword_size; /* :34 */
    void* stream;
} gr4pm_syncword_remove_params;
gr4pm_status gr4pm_syncword_remove_create(const gr4pm_syncword_remove_params* params,
                                          gr4pm_syncword_remove** out);
void gr4pm_syncword_remove_destroy(gr4pm_syncword_remove* h);
gr4pm_status gr4pm_syncword_remove_reset(gr4pm_syncword_remove* h);
/* out holds n - (dropped syncword items) <= n items; GR4PM_PKT_SYNCWORD tags start a syncword
 * and are swallowed (:51-58), the others pass, re-indexed (:59-62). */
gr4pm_status gr4pm_syncword_remove_process(gr4pm_syncword_remove* h, const gr4pm_c64* in, size_t n,
                                           gr4pm_c64* out, const gr4pm_packet_tag* tags_in,
                                           size_t n_tags_in, gr4pm_packet_tag* tags_out, size_t tags_cap,
                                           size_t* n_tags_out, size_t* produced);

/* ------------------------------------------------------------------------------------
 * ConstellationLLRDecoder<float> -- constellation_llr_decoder.hpp:13-142
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_constellation_llr_decoder gr4pm_constellation_llr_decoder;
typedef struct {
    float noise_sigma; /* :45 */
    int constellation; /* :46-47: 1 BPSK, 2 QPSK (0 PILOT is rejected like :72-74) */
    void* stream;
} gr4pm_constellation_llr_decoder_params;
gr4pm_status gr4pm_constellation_llr_decoder_create(const gr4pm_constellation_llr_decoder_params* params,
                                                    gr4pm_constellation_llr_decoder** out);
void gr4pm_constellation_llr_decoder_destroy(gr4pm_constellation_llr_decoder* h);
/* out: device floats, out_cap >= 2 n is always enough.  "constellation" keys switch the mapping
 * from the tagged item on; tags leave at the LLR index of their item (:93-99). */
gr4pm_status gr4pm_constellation_llr_decoder_process(gr4pm_constellation_llr_decoder* h, const gr4pm_c64* in,
                                                     size_t n, float* out, size_t out_cap,
                                                     const gr4pm_packet_tag* tags_in, size_t n_tags_in,
                                                     gr4pm_packet_tag* tags_out, size_t tags_cap,
                                                     size_t* n_tags_out, size_t* produced);

/* ====================================================================================
 * Header decode loop (packet_receiver.hpp:131-139): descrambler ->
 * header/payload split -> header FEC decoder -> header parser.  It produces the parsed_header
 * messages SyncwordDetectionFilter and PayloadMetadataInsert wait for.
 * ================================================================================== */

/* ------------------------------------------------------------------------------------
 * AdditiveScrambler<float | uint8_t> -- additive_scrambler.hpp:24-100
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_additive_scrambler gr4pm_additive_scrambler;
typedef struct {
    uint64_t mask;   /* :61 */
    uint64_t seed;   /* :62 */
    uint64_t length; /* :63 */
    uint64_t count;  /* :64, 0 = never reset by count */
    int item_kind;   /* 1: float soft symbols (sign flip), 2: uint8_t hard symbols (XOR) */
    void* stream;
} gr4pm_additive_scrambler_params;
gr4pm_status gr4pm_additive_scrambler_create(const gr4pm_additive_scrambler_params* params,
                                             gr4pm_additive_scrambler** out);
void gr4pm_additive_scrambler_destroy(gr4pm_additive_scrambler* h);
gr4pm_status gr4pm_additive_scrambler_reset(gr4pm_additive_scrambler* h); /* start(), :68 */
/* reset_index: host, sorted item indices that carry the reset_tag_key (:78-83) */
gr4pm_status gr4pm_additive_scrambler_process(gr4pm_additive_scrambler* h, const void* in, size_t n,
                                              void* out, const uint64_t* reset_index, size_t n_resets);

/* ------------------------------------------------------------------------------------
 * HeaderPayloadSplit<float> -- header_payload_split.hpp:9-147
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_header_payload_split gr4pm_header_payload_split;
typedef struct {
    size_t header_size; /* :33 */
    void* stream;
} gr4pm_header_payload_split_params;
gr4pm_status gr4pm_header_payload_split_create(const gr4pm_header_payload_split_params* params,
                                               gr4pm_header_payload_split** out);
void gr4pm_header_payload_split_destroy(gr4pm_header_payload_split* h);
gr4pm_status gr4pm_header_payload_split_reset(gr4pm_header_payload_split* h); /* start(), :41-45 */
/* GR4PM_PKT_PAYLOAD tags carry "payload_bits" (:70-82).  header / payload: device, each with
 * room for n items.  Tags leave on the output their item goes to (:83-87).  A payload tag in
 * the wrong place is the reference's exception (:75-78): GR4PM_ERR_INVALID. */
gr4pm_status gr4pm_header_payload_split_process(gr4pm_header_payload_split* h, const float* in, size_t n,
                                                float* header, size_t* n_header, float* payload,
                                                size_t* n_payload, const gr4pm_packet_tag* tags_in,
                                                size_t n_tags_in, gr4pm_packet_tag* header_tags,
                                                size_t* n_header_tags, gr4pm_packet_tag* payload_tags,
                                                size_t* n_payload_tags, size_t tags_cap);
/* HeaderPayloadSplit<std::complex<float>>: the split of the symbol tap, packet_receiver.hpp:159-162 (header_size 128,
 * the GR4PM_PKT_PAYLOAD tags then carry "payload_symbols" in payload_bits).  Same state machine, complex items. */
gr4pm_status gr4pm_header_payload_split_process_c64(gr4pm_header_payload_split* h, const gr4pm_c64* in, size_t n,
                                                    gr4pm_c64* header, size_t* n_header, gr4pm_c64* payload,
                                                    size_t* n_payload, const gr4pm_packet_tag* tags_in,
                                                    size_t n_tags_in, gr4pm_packet_tag* header_tags,
                                                    size_t* n_header_tags, gr4pm_packet_tag* payload_tags,
                                                    size_t* n_payload_tags, size_t tags_cap);

/* ------------------------------------------------------------------------------------
 * HeaderFecDecoder -- header_fec_decoder.hpp:13-359: 256 LLRs (rate-1/2 repetition of a
 * (128, 32) LDPC codeword) -> 4 header bytes, or "invalid_header".
 * The reference hands the LDPC decoding to its Rust dependency ldpc-toolbox
 * (ldpc_toolbox_decoder_ctor_alist_string(alist, "HLAminstari8", ""), :276, and
 * ldpc_toolbox_decoder_decode_f32, :315-321, 25 iterations).  `alist` is that same string.
 * The decoder itself takes any (n, m) code with n <= 256, m <= 192, row weight 1 ... 8, no variable twice in a row,
 * n - m a multiple of 8 up to 64 and a layering of at most 24 steps (create refuses the rest): 2 n LLRs ->
 * (n - m) / 8 bytes per codeword, gr4pm_header_fec_decoder_dims.
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_header_fec_decoder gr4pm_header_fec_decoder;
typedef struct {
    const char* alist;       /* parity-check matrix, alist text (:31-258) */
    uint32_t max_iterations; /* :314, 25 */
    void* stream;
    int arithmetic;          /* message arithmetic of the horizontal-layered A-Min* decoder ("HLAminstari8": HL =
                                horizontal-layered schedule, Aminstar = the A-Min* check-node rule, i8 = 8-bit messages):
                                0 (default) float32 messages; 1 the same schedule and rule with 8-bit messages -- LLRs in
                                eighths, channel LLRs and messages saturating at +-127.  The crate is not part of the
                                reference tree, so neither form is pinned against it bit for bit; form 1 exists to show
                                what 8-bit messages change (tests/test_gpu_parity.py: frame-error rates side by side). */
} gr4pm_header_fec_decoder_params;
gr4pm_status gr4pm_header_fec_decoder_create(const gr4pm_header_fec_decoder_params* params,
                                             gr4pm_header_fec_decoder** out);
void gr4pm_header_fec_decoder_destroy(gr4pm_header_fec_decoder* h);
/* The sizes of one codeword of the handle's (n, m) code: 2 n LLRs in (the codeword twice, :308-312) and (n - m) / 8
 * header bytes out -- 256 and 4 for the header code.  Either pointer may be NULL.  A caller whose buffers are built
 * for one code asks here after create and refuses every other code. */
gr4pm_status gr4pm_header_fec_decoder_dims(const gr4pm_header_fec_decoder* h, size_t* llrs_per_codeword,
                                           size_t* header_bytes);
/* llrs: device, 2 n per codeword.  headers: host, (n - m) / 8 bytes per codeword; invalid: host, one
 * flag per codeword (the "invalid_header" tag of :322-326).  See gr4pm_header_fec_decoder_dims. */
gr4pm_status gr4pm_header_fec_decoder_process(gr4pm_header_fec_decoder* h, const float* llrs,
                                              size_t n_codewords, uint8_t* headers, uint8_t* invalid);

/* HeaderParser -- header_parser.hpp:46-95 (host): 4 bytes (+ the decoder's verdict) -> the
 * parsed_header message; packet_type: 0 USER_DATA, 1 IDLE, -1 when invalid. */
void gr4pm_header_parse(const uint8_t* headers, const uint8_t* invalid, size_t n, gr4pm_header_msg* msgs,
                        int32_t* packet_type);

/* ====================================================================================
 * Payload tail (packet_receiver.hpp:140-147): BinarySlicer<true> -> PackBits<> -> CrcCheck<>.
 * ================================================================================== */

/* BinarySlicer<invert, float, uint8_t> -- binary_slicer.hpp:10-35: out = invert ? in < 0 : in > 0 */
gr4pm_status gr4pm_binary_slicer_process(const float* in, size_t n, uint8_t* out, int invert, void* stream);
/* PackBits<MSB|LSB, uint8_t, uint8_t> -- pack_bits.hpp: n_out outputs, each joins
 * inputs_per_output inputs of bits_per_input bits (inputs_per_output * bits_per_input <= 8) */
gr4pm_status gr4pm_pack_bits_process(const uint8_t* in, size_t n_out, uint8_t* out, size_t inputs_per_output,
                                     unsigned bits_per_input, int msb_first, void* stream);
/* both at once for the receiver's wiring (invert = true, 8 x 1 bit, MSB first): n_out bytes from
 * 8 n_out soft bits */
gr4pm_status gr4pm_slice_pack_process(const float* in, size_t n_out, uint8_t* out, void* stream);

/* CrcCheck<uint64_t> -- crc_check.hpp:22-239 with Crc<uint64_t> -- crc.hpp:31-156 */
typedef struct gr4pm_crc_check gr4pm_crc_check;
typedef struct {
    unsigned num_bits;          /* crc_check.hpp:61, multiple of 8 */
    uint64_t poly;              /* :62 */
    uint64_t initial_value;     /* :63 */
    uint64_t final_xor;         /* :64 */
    int input_reflected;        /* :65 */
    int result_reflected;       /* :66 */
    int swap_endianness;        /* :67 */
    int discard_crc;            /* :68 */
    uint64_t skip_header_bytes; /* :69 */
    void* stream;
} gr4pm_crc_check_params;
gr4pm_status gr4pm_crc_check_create(const gr4pm_crc_check_params* params, gr4pm_crc_check** out);
void gr4pm_crc_check_destroy(gr4pm_crc_check* h);
/* host helper: Crc::compute over host bytes (crc.hpp:119-156) */
uint64_t gr4pm_crc_check_compute(const gr4pm_crc_check* h, const uint8_t* data, size_t n);
/* in: device bytes; packet i occupies [packet_offset[i], packet_offset[i] + packet_len[i]) ("packet_len"
 * tags).  Packets whose CRC matches are copied to `out` (device) back to back, without the CRC
 * when discard_crc; out_len[i] (host) = bytes written for packet i, 0 = dropped (:152-208). */
gr4pm_status gr4pm_crc_check_process(gr4pm_crc_check* h, const uint8_t* in, const uint64_t* packet_offset,
                                     const uint64_t* packet_len, size_t n_packets, uint8_t* out,
                                     uint64_t* out_len, size_t* n_out_bytes);

/* ====================================================================================
 * PacketReceiver -- packet_receiver.hpp:34-147,191-247: the composition itself, native.
 * The reference wires the blocks into a flowgraph and runs them with the multi-threaded
 * scheduler (one worker per block).  This object owns the blocks of the chain up to the Costas
 * loop (soft_bits: up to the LLR decoder; decode_headers: the whole receiver), its HIP streams and
 * worker threads; batches are submitted and collected, up to four in flight:
 *   stage 0 (caller's thread, inside submit): SyncwordDetection (+ look-ahead of the next batch)
 *   stage 1: SyncwordDetectionFilter gate, CoarseFrequencyCorrection + SymbolFilter, SyncwordWipeoff
 *   stage 2: CostasLoop [PayloadMetadataInsert, tag-driven CostasLoop, SyncwordRemove, LLR decoder]
 *   stage 3 (decode_headers): descrambler, HeaderPayloadSplit, HeaderFecDecoder, HeaderParser,
 *            BinarySlicer, PackBits, CrcCheck
 * The parsed_header feedback is a constant packet_length per submit (0 = every header invalid),
 * or with decode_headers the header decode loop on the device.
 * ================================================================================== */
/* The symbol PDU tap of packet_receiver.hpp:159-189 (`zmq_output`): SyncwordRemove's output ->
 * HeaderPayloadSplit<c64>{ header_size 128, payload_length_key "payload_symbols" } -> TaggedStreamToPdu ->
 * ZmqPduPubSink on TCP port 5000 (headers) / :5001 (payloads).  The split (header_payload_split.hpp:46-135) is done by
 * the receiver: every batch's post-SyncwordRemove symbols are cut into header PDUs (128 symbols) and payload PDUs
 * ("payload_symbols" symbols behind a parsed header); a PDU that crosses a batch boundary appears as a piece with
 * `last == 0` and continues in the next batch with `first == 0`.  With a callback registered, collect() copies the
 * batch's symbols to the host once and calls it once per COMPLETE PDU, in stream order, from the collecting thread:
 * the place where a caller publishes them (gr4pm_packet_receiver_publish_symbol_pdus below does: ZMTP 3.0, no libzmq). */
typedef struct {
    uint64_t offset;  /* first symbol of the piece inside pdu_symbols */
    uint64_t length;  /* symbols of the piece in this batch */
    int32_t kind;     /* 0 header, 1 payload */
    int32_t first;    /* the PDU starts with this piece */
    int32_t last;     /* the PDU ends with this piece */
    int32_t pad;
} gr4pm_symbol_pdu;
typedef void (*gr4pm_symbol_pdu_fn)(void* user, int kind, const gr4pm_c64* symbols_host, size_t n_symbols);
typedef struct gr4pm_packet_receiver gr4pm_packet_receiver;
typedef struct {
    size_t samples_per_symbol; /* packet_receiver.hpp:49 */
    int syncword_freq_bins;    /* :54 */
    float syncword_threshold;  /* :55 */
    int costas_constellation;  /* CostasLoop setting when soft_bits == 0 (0 PILOT 1 BPSK 2 QPSK) */
    size_t max_items;          /* largest batch */
    size_t tags_cap;           /* most detections per batch */
    int pipelined;             /* 0: submit() runs the three stages itself */
    int soft_bits;             /* continue to the LLR decoder (:123-131) */
    int decode_headers;        /* (needs soft_bits and samples_per_symbol >= 4: create refuses the mode below that with
                                  GR4PM_ERR_INVALID) close the header feedback loop on the device and run the
                                  payload tail: descrambler, HeaderPayloadSplit, HeaderFecDecoder, HeaderParser
                                  (:131-139) answer SyncwordDetectionFilter and PayloadMetadataInsert instead of
                                  packet_length; BinarySlicer, PackBits, CrcCheck (:140-147) deliver the packets.
                                  Two passes per batch, see HISTORY.md 5c. */
    const char* header_alist;  /* decode_headers: the header code, header_fec_decoder.hpp:31-258 */
    int packets_only;          /* (decode_headers) round 6: what benchmarks/benchmark_packet_receiver.cpp measures -- IQ in,
                                  CRC-checked packets out -- with the stream between the Costas loop and the packer never
                                  written to memory: SyncwordRemove, the LLR decoder, the descrambler, HeaderPayloadSplit,
                                  the slicer and the packer advance their state on the host as always, and ONE kernel
                                  (k_tail_fused) reads every Costas-loop output symbol once, writes header LLRs for the
                                  header decoder and packed payload bytes for CrcCheck.  The same packets, header messages
                                  and tags as the full form, bit for bit; result.llr, .payload_llr and .pdu_symbols are NULL
                                  (their counts and tags are still reported), out_llr may be NULL, no symbol PDU tap. */
} gr4pm_packet_receiver_params;
typedef struct {
    size_t consumed;                    /* items of the batch SyncwordDetection consumed */
    const gr4pm_c64* symbols;           /* == out_symbols of the submit */
    size_t n_symbols;
    const float* llr;                   /* == out_llr of the submit (soft_bits) */
    size_t n_llr;
    const gr4pm_tag* detector_tags;     /* host; valid until the next collect() */
    size_t n_detector_tags;
    const uint8_t* accepted;            /* per detector tag: passed the filter */
    const gr4pm_tag* tags;              /* symbol-rate tags of the accepted detections */
    size_t n_tags;
    const gr4pm_packet_tag* packet_tags; /* soft_bits: PayloadMetadataInsert's tags (symbol index) */
    size_t n_packet_tags;
    const gr4pm_packet_tag* llr_tags;   /* soft_bits: tags at LLR positions */
    size_t n_llr_tags;
    size_t ignored_syncwords;
    /* decode_headers */
    const gr4pm_header_msg* header_messages; /* the headers the chain decoded in this batch, in order */
    const int32_t* packet_type;
    size_t n_header_messages;
    size_t header_mismatches;           /* of those, how many differ from the message pass A had supplied */
    const float* payload_llr;           /* device: descrambled payload LLRs of this batch */
    size_t n_payload_llr;
    const gr4pm_packet_tag* payload_tags;
    size_t n_payload_tags;
    const uint8_t* packets;             /* == out_packets: bytes of the packets whose CRC-32 matches */
    size_t n_packet_bytes;
    const uint64_t* packet_lengths;     /* per finished packet: bytes delivered, 0 = CRC failure */
    size_t n_packets;
    /* soft_bits: the symbol PDU tap (below) */
    const gr4pm_c64* pdu_symbols;       /* device: SyncwordRemove's output of this batch (header + payload symbols) */
    size_t n_pdu_symbols;
    const gr4pm_symbol_pdu* symbol_pdus; /* host: the pieces of header / payload PDUs inside pdu_symbols, in order */
    size_t n_symbol_pdus;
    size_t symbol_pdu_resyncs;          /* "payload_symbols" tags that arrived where the tap's HeaderPayloadSplit did not
                                           expect one (the reference block throws, header_payload_split.hpp:75-78; here
                                           the tap starts over at the tag and the batch -- LLRs, packets -- is not failed
                                           because of its optional side output) */
} gr4pm_packet_receiver_result;
gr4pm_status gr4pm_packet_receiver_create(const gr4pm_packet_receiver_params* params,
                                          gr4pm_packet_receiver** out);
void gr4pm_packet_receiver_destroy(gr4pm_packet_receiver* h);
/* in: device, n_in items.  delayed: NULL, or the address of item -(2 time_threshold + 1) of the
 * stream relative to in[0] when `in` is a window of a device ring (the chain then reads the
 * delayed stream in place).  next_in/next_n: the following batch (look-ahead) or NULL.
 * out_symbols (device, out_cap >= n_in / samples_per_symbol + tags + 2) and out_llr (device,
 * soft_bits, 2 floats per symbol) and out_packets (device, decode_headers; a QPSK stream carries at most
 * n_in / (4 samples_per_symbol) payload bytes, n_in / 16 at the lowest rate that decode_headers takes, plus the
 * packet a batch finishes for the one before) stay the caller's; the result points at them.  decode_headers: a batch
 * has at least (228 + 16) samples_per_symbol + 2048 items (3024 at 4 samples per symbol) -- the first pass decodes
 * every detection's header from a window of 228 symbols that begins 16 symbols in front of the tag; a shorter batch
 * is refused with GR4PM_ERR_INVALID.  The receiver works on streams of its
 * own, which are not ordered against the caller's: `in` (and `next_in`, and what announce names) must be
 * complete when the call is made. */
gr4pm_status gr4pm_packet_receiver_submit(gr4pm_packet_receiver* h, const gr4pm_c64* in, size_t n_in,
                                          const gr4pm_c64* delayed, const gr4pm_c64* next_in,
                                          size_t next_n, uint64_t packet_length, gr4pm_c64* out_symbols,
                                          size_t out_cap, float* out_llr, size_t llr_cap, uint8_t* out_packets,
                                          size_t packets_cap);
/* names the input of a later submit (after the ones already announced): forwarded to the
 * detector's look-ahead, gr4pm_syncword_detection_announce; next_in of _submit is the one-call
 * form (gr4pm_syncword_detection_hint_next) */
gr4pm_status gr4pm_packet_receiver_announce(gr4pm_packet_receiver* h, const gr4pm_c64* in, size_t n_in);
/* waits for the oldest batch; returns its status (the error text of a failed stage included) */
gr4pm_status gr4pm_packet_receiver_collect(gr4pm_packet_receiver* h, gr4pm_packet_receiver_result* result);
size_t gr4pm_packet_receiver_inflight(const gr4pm_packet_receiver* h);
/* the most batches _submit accepts in flight (a further _submit fails until one is collected): a caller that recycles
 * its output buffers needs more sets than this */
size_t gr4pm_packet_receiver_max_inflight(void);
/* soft_bits receivers: fn == NULL removes the callback */
gr4pm_status gr4pm_packet_receiver_set_symbol_pdu_callback(gr4pm_packet_receiver* h, gr4pm_symbol_pdu_fn fn, void* user);

/* ------------------------------------------------------------------------------------
 * ZmqPduPubSink<T> -- zmq_pdu_pub_sink.hpp:11-44: a ZeroMQ PUB socket, one message per PDU holding its raw items.
 * The library speaks ZMTP 3.0 (NULL mechanism) itself -- greeting, READY, the subscriptions a SUB peer sends, one
 * single-frame message per send, PUB drop semantics (no subscriber / a peer whose queue holds 1000 messages) -- so a
 * zmq.SUB socket (scripts/plot_symbols.py:10-17) connects to it as to the reference's; libzmq is not needed.
 * Host only: works without a HIP device.
 * ---------------------------------------------------------------------------------- */
typedef struct gr4pm_zmq_pub gr4pm_zmq_pub;
/* endpoint (:26): tcp://HOST:PORT as ZeroMQ spells it -- HOST an IPv4 address or a star (every interface), PORT a
 * number, or a star / 0 for an ephemeral port (gr4pm_zmq_pub_port); the reference's default is port 5555 on every interface.
 * = start(): socket.bind(endpoint) (:29) */
gr4pm_status gr4pm_zmq_pub_create(const char* endpoint, gr4pm_zmq_pub** out);
void gr4pm_zmq_pub_destroy(gr4pm_zmq_pub* h); /* queued messages get 200 ms to leave */
/* processOne() (:31-41): data = a PDU's items (host), one message; never blocks on a peer */
gr4pm_status gr4pm_zmq_pub_send(gr4pm_zmq_pub* h, const void* data, size_t bytes);
int gr4pm_zmq_pub_port(const gr4pm_zmq_pub* h);           /* the bound TCP port */
size_t gr4pm_zmq_pub_subscribers(const gr4pm_zmq_pub* h); /* connected peers holding a subscription */
uint64_t gr4pm_zmq_pub_dropped(const gr4pm_zmq_pub* h);   /* messages a subscribed peer did not get: its queue was full */
/* packet_receiver.hpp:159-189 (`zmq_output`) in one call: header PDUs to header_endpoint (port 5000 on every interface, :166),
 * payload PDUs to payload_endpoint (port 5001, :168), published by collect() (it takes the place of a callback set
 * with gr4pm_packet_receiver_set_symbol_pdu_callback, and is removed by one).  NULL, NULL stops publishing.  `ports`
 * (may be NULL): the two bound TCP ports. */
gr4pm_status gr4pm_packet_receiver_publish_symbol_pdus(gr4pm_packet_receiver* h, const char* header_endpoint,
                                                       const char* payload_endpoint, int ports[2]);

/* gr4pm_multichannel_receiver: BASELINE configs[2] -- n_channels independent receive chains on one
 * GPU (front-end mode of gr4pm_packet_receiver, channel by channel).  One batched
 * SyncwordDetection handle for all channels, then every channel's own SyncwordDetectionFilter /
 * CoarseFrequencyCorrection / SymbolFilter / SyncwordWipeoff / CostasLoop, spread over `workers`
 * threads with a stream each.  process() is synchronous; submit() / collect() run the same chain as a
 * pipeline: submit returns when the detector has consumed the batch, the stages behind it (tag gates + CFC
 * plan | symbol filters + wipe-off | Costas loop) work on up to GR4PM_MC_SLOTS batches at a time in their own
 * threads, collect() waits for the oldest one (results in submission order, bit-identical to process()). */
#define GR4PM_MC_SLOTS 4
typedef struct gr4pm_multichannel_receiver gr4pm_multichannel_receiver;
typedef struct {
    size_t n_channels;
    size_t samples_per_symbol;
    int syncword_freq_bins;
    float syncword_threshold;
    int costas_constellation; /* 0 PILOT, 1 BPSK, 2 QPSK */
    size_t max_items;         /* per channel and call */
    size_t tags_cap;          /* per channel and call */
    int workers;
} gr4pm_multichannel_receiver_params;
gr4pm_status gr4pm_multichannel_receiver_create(const gr4pm_multichannel_receiver_params* params,
                                                gr4pm_multichannel_receiver** out);
void gr4pm_multichannel_receiver_destroy(gr4pm_multichannel_receiver* h);
/* the detector's look-ahead (gr4pm_syncword_detection_announce) */
gr4pm_status gr4pm_multichannel_receiver_announce(gr4pm_multichannel_receiver* h, const gr4pm_c64* in,
                                                  size_t in_stride, size_t n_in);
/* in: device [n_channels][in_stride], n_in items per channel.  packet_length: the parsed_header
 * answer for every packet (0: "invalid_header").  out_symbols: device [n_channels][out_stride]
 * (out_stride >= n_in / samples_per_symbol + tags + 2); n_symbols, n_tags, n_detector_tags: host
 * [n_channels]; tags, detector_tags: host [n_channels][tags_cap] (may be NULL). */
gr4pm_status gr4pm_multichannel_receiver_process(gr4pm_multichannel_receiver* h, const gr4pm_c64* in,
                                                 size_t in_stride, size_t n_in, uint64_t packet_length,
                                                 gr4pm_c64* out_symbols, size_t out_stride, size_t* consumed,
                                                 size_t* n_symbols, gr4pm_tag* tags, size_t* n_tags,
                                                 gr4pm_tag* detector_tags, size_t* n_detector_tags);

/* the pipelined form: out_symbols must stay valid until the batch has been collected.  The receiver works on
 * streams of its own, which are not ordered against the caller's: `in` must be complete (its producer finished,
 * or waited for) when submit / announce is called. */
gr4pm_status gr4pm_multichannel_receiver_submit(gr4pm_multichannel_receiver* h, const gr4pm_c64* in,
                                                size_t in_stride, size_t n_in, uint64_t packet_length,
                                                gr4pm_c64* out_symbols, size_t out_stride, size_t* consumed);
gr4pm_status gr4pm_multichannel_receiver_collect(gr4pm_multichannel_receiver* h, size_t* consumed, size_t* n_symbols,
                                                 gr4pm_tag* tags, size_t* n_tags, gr4pm_tag* detector_tags,
                                                 size_t* n_detector_tags);
int gr4pm_multichannel_receiver_in_flight(const gr4pm_multichannel_receiver* h);
/* on: the caller keeps every submitted input valid and unchanged until its batch has been collected (a device
 * ring).  SyncwordDetection's output is its input delayed by 2 * time_threshold + 1 items
 * (syncword_detection.hpp:318-319,342).  The receiver then reads SyncwordDetection's delayed stream in place (the tail of the batch before, kept
 * by the receiver, + the batch's own input) instead of writing a delayed copy of every batch (16 B/sample).
 * Same results.  Call it before the first batch. */
gr4pm_status gr4pm_multichannel_receiver_set_input_in_place(gr4pm_multichannel_receiver* h, int on);

/* ====================================================================================
 * Burst generator pieces (packet_transmitter_pdu.hpp:131-337): with
 * AdditiveScrambler, PackBits, InterpolatingFirFilter, Rotator and PfbArbResampler above they
 * build the test signal on the device.
 * ================================================================================== */
/* Mapper<uint8_t, c64 | float> -- mapper.hpp:13-51: out[i] = map[in[i] & (map_size - 1)];
 * map_size must be a power of two (:37-41); item_kind 0: c64 map/out, 1: float. */
gr4pm_status gr4pm_mapper_process(const uint8_t* in, size_t n, void* out, const void* map_host,
                                  size_t map_size, int item_kind, void* stream);
/* BurstShaper<c64 | float, ., float> -- burst_shaper.hpp:47-126: the first leading_n items of
 * every packet are multiplied by leading[], the last trailing_n by trailing[] (short packets:
 * leading first, :98-124).  Packets: [packet_offset[i], + packet_len[i]) ("packet_len" tags),
 * whole packets per call; items outside packets are copied. */
gr4pm_status gr4pm_burst_shaper_process(const void* in, size_t n, void* out, int item_kind,
                                        const float* leading_host, size_t leading_n,
                                        const float* trailing_host, size_t trailing_n,
                                        const uint64_t* packet_offset, const uint64_t* packet_len,
                                        size_t n_packets, void* stream);

/* The library's cosf / sinf on device arrays: the local oscillator of CostasLoop (costas_loop.hpp:113-115 calls
 * std::cos(float) / std::sin(float), i.e. glibc's cosf / sinf; the kernels restate glibc's double-precision
 * algorithm and are bit-exact with it for |x| < 120).  Exposed so that the parity suite can pin it directly. */
gr4pm_status gr4pm_sincosf(const float* x, size_t n, float* sin_out, float* cos_out);

/* The phase wrap at the end of a CostasLoop iteration on device arrays -- costas_loop.hpp:141-145
 * (`if (phase >= pi) phase -= 2 pi; else if (phase < -pi) phase += 2 pi`, float).  The kernels evaluate it without
 * compares (two fused multiply-adds with the clamp modifier); exposed so that the parity suite can pin it on the
 * boundary values a signal rarely produces. */
gr4pm_status gr4pm_costas_phase_wrap(const float* x, size_t n, float* out);

/* firdes::root_raised_cosine<float> -- firdes.hpp:29-76 (host helper; out: ntaps|1 floats) */
size_t gr4pm_firdes_root_raised_cosine(double gain, double sampling_freq, double symbol_rate,
                                       double alpha, size_t ntaps, float* out);

/* ====================================================================================
 * PacketTransmitterPdu -- packet_transmitter_pdu.hpp:40-355: payload bytes to IQ.
 * Burst mode (stream_mode = 0): one burst per packet of samples_per_symbol * (4 L + 228) samples
 * (L = payload bytes): syncword (64 BPSK), the scrambled header (LDPC(128,32) code word twice) and
 * payload + big-endian CRC-32 (QPSK), 9 ramp-down symbols from a degree-32 GlfsrSource (seed 1,
 * carried across bursts and calls until reset()), 11 zero symbols; interpolated by the transmitter's
 * RRC (packet_transmitter_rrc_taps.hpp) and shaped by sine ramps (BurstShaper).  Optional gaps of
 * zeros in front of each burst.  Stream mode: syncword, header and payload only, back to back through
 * one filter whose history carries over to the next call.
 * ================================================================================== */
typedef struct gr4pm_packet_transmitter gr4pm_packet_transmitter;
typedef struct {
    size_t samples_per_symbol;          /* default 4; 1..64 */
    int stream_mode;                    /* packet_transmitter_pdu.hpp:41 */
    size_t max_packets;                 /* per process() call */
    size_t max_payload_bytes;           /* per process() call, all packets together */
    const uint32_t* header_generator;   /* host: the 96 rows of the header's LDPC(128,32) generator
                                           (data/header_ldpc_generator.u32), copied at create */
    void* stream;                       /* hipStream_t (NULL: the default stream) */
} gr4pm_packet_transmitter_params;
gr4pm_status gr4pm_packet_transmitter_create(const gr4pm_packet_transmitter_params* params,
                                             gr4pm_packet_transmitter** out);
void gr4pm_packet_transmitter_destroy(gr4pm_packet_transmitter* h);
/* the GLFSR back to its seed, the stream mode filter history to zeros */
gr4pm_status gr4pm_packet_transmitter_reset(gr4pm_packet_transmitter* h);
/* samples process() writes for these packets (host arrays as in process()), with the same checks */
gr4pm_status gr4pm_packet_transmitter_output_items(const gr4pm_packet_transmitter* h, const uint64_t* lengths,
                                                   const uint8_t* packet_types, const uint64_t* gaps,
                                                   size_t n_packets, size_t* n_out);
/* payload: DEVICE bytes of the n_packets packets back to back; lengths: host, 1..65535 each;
 * packet_types: host, 0 USER_DATA / 1 IDLE (NULL: all USER_DATA); gaps: host, samples of silence in
 * front of each burst (NULL: none; burst mode only).  out: DEVICE c64, out_cap items.  Host outputs:
 * burst_offsets[i] / burst_lengths[i] (the "packet_len" tags) and n_out.  A length of 0 (PacketIngress
 * throws, packet_ingress.hpp:171-172) or above 65535 (HeaderFormatter, header_formatter.hpp:102-106),
 * an unknown packet type, gaps in stream mode (GR4PM_ERR_INVALID), more packets or payload bytes than
 * the handle was made for, or an out_cap below the samples of the call (GR4PM_ERR_OVERFLOW) are
 * refused before anything is written. */
gr4pm_status gr4pm_packet_transmitter_process(gr4pm_packet_transmitter* h, const uint8_t* payload,
                                              const uint64_t* lengths, const uint8_t* packet_types,
                                              const uint64_t* gaps, size_t n_packets, gr4pm_c64* out,
                                              size_t out_cap, uint64_t* burst_offsets, uint64_t* burst_lengths,
                                              size_t* n_out);

/* ====================================================================================
 * NoiseSource<T> -- noise_source.hpp:45-110 over random.hpp / xoroshiro128p.h: the reference's
 * sequential stream bit for bit (ROCm clang++ against libstdc++: generate_canonical<float, 24>
 * with the clamp of 1.0, std::complex(gasdev(), gasdev()) evaluated left to right), generated in
 * parallel for any call size and any chain of calls.  Seed 0 is an ordinary seed.  Complex items
 * take UNIFORM and GAUSSIAN only.  The stream position stays on the device: process() enqueues on
 * the handle's stream and does not wait.
 * ================================================================================== */
#define GR4PM_NOISE_C64 0
#define GR4PM_NOISE_FLOAT 1
#define GR4PM_NOISE_UNIFORM 0
#define GR4PM_NOISE_GAUSSIAN 1
#define GR4PM_NOISE_LAPLACIAN 2
#define GR4PM_NOISE_IMPULSE 3
typedef struct gr4pm_noise_source gr4pm_noise_source;
typedef struct {
    int item_kind;      /* GR4PM_NOISE_C64 (gr4pm_c64 items) or GR4PM_NOISE_FLOAT */
    int noise_type;     /* GR4PM_NOISE_UNIFORM / GAUSSIAN / LAPLACIAN / IMPULSE (the reference's NoiseType) */
    float amplitude;    /* complex items: amplitude / sqrt2_v<float> per component */
    uint64_t seed;      /* random(seed) at start() */
    size_t max_items;   /* per process() call; 1..2^31 */
    void* stream;       /* hipStream_t (NULL: the default stream) */
} gr4pm_noise_source_params;
gr4pm_status gr4pm_noise_source_create(const gr4pm_noise_source_params* params, gr4pm_noise_source** out);
void gr4pm_noise_source_destroy(gr4pm_noise_source* h);
/* back to the start of the stream (start(): random(seed)) */
gr4pm_status gr4pm_noise_source_reset(gr4pm_noise_source* h);
/* settingsChanged: the amplitude of later items; the stream position is kept */
gr4pm_status gr4pm_noise_source_set_amplitude(gr4pm_noise_source* h, float amplitude);
/* the next n items into out (DEVICE, gr4pm_c64 or float as the handle's item_kind).  add_in: NULL for
 * the noise alone, or DEVICE items of the same kind: out = add_in + noise (Add::processOne(signal,
 * noise)); add_in may be out.  More than max_items is refused before anything is written. */
gr4pm_status gr4pm_noise_source_process(gr4pm_noise_source* h, const void* add_in, void* out, size_t n);
/* glibc's logf as the noise kernels compute it (DEVICE x, out; synchronous) */
gr4pm_status gr4pm_logf(const float* x, size_t n, float* out);

/* ====================================================================================
 * Channelizer -- critically sampled polyphase analysis bank (the project's own block: the reference
 * is a one-channel modem).  One wideband c64 stream at fs becomes M channels at fs / M, channel-major,
 * in the layout gr4pm_multichannel_receiver_submit takes.  With a real prototype h[0 .. P M - 1] and
 * x[i] = 0 for i < 0 (a fresh handle, or after reset()):
 *     z_k[i] = x[i] exp(-2 pi j k i / M),   w_k = h * z_k,   y_k[n] = w_k[n M + M - 1]
 * Channel k sits at +k fs / M (k > M / 2: negative frequencies, as an FFT orders them).  Plain float32,
 * every product and sum rounded on its own in an order that does not depend on how the stream is cut
 * into calls.  M: a power of two in [2, 1024]; P: 1 .. 32.  The last (P - 1) M samples and the samples
 * of an incomplete frame stay in the handle on the device: process() takes any n_in, enqueues on the
 * handle's stream and does not wait.
 * ================================================================================== */
typedef struct gr4pm_channelizer gr4pm_channelizer;
typedef struct {
    size_t n_channels;       /* M */
    size_t taps_per_branch;  /* P */
    const float* taps;       /* host: P M prototype taps, copied at create (NULL: the default design,
                                gr4pm_channelizer_taps(M, P, 0.25, 0.75)) */
    size_t n_select;         /* 0: all M rows in order; else the rows to write, in this order */
    const uint32_t* select;  /* host: n_select channel numbers, each < M, no duplicates */
    size_t max_frames;       /* per process() call: n_in <= max_frames M; 1..2^31 */
    void* stream;            /* hipStream_t (NULL: the default stream) */
} gr4pm_channelizer_params;
/* Kaiser-windowed sinc designed in double and rounded to float once, DC gain 1 (host only: no device
 * needed).  passband / stopband: the band edges in units of the channel spacing fs / M; the cutoff is
 * midway, the window's beta follows from the attenuation Kaiser's length rule gives P M taps over that
 * transition.  out: P M floats. */
gr4pm_status gr4pm_channelizer_taps(size_t n_channels, size_t taps_per_branch, double passband, double stopband,
                                    float* out);
gr4pm_status gr4pm_channelizer_create(const gr4pm_channelizer_params* params, gr4pm_channelizer** out);
void gr4pm_channelizer_destroy(gr4pm_channelizer* h);
/* back to the fresh stream: zero history, no carried samples */
gr4pm_status gr4pm_channelizer_reset(gr4pm_channelizer* h);
/* frames the next process() of n_in samples produces; the state is unchanged */
gr4pm_status gr4pm_channelizer_output_items(const gr4pm_channelizer* h, size_t n_in, size_t* n_frames);
/* in: DEVICE, n_in samples (any number; all are consumed).  out: DEVICE, row r (channel r, or
 * select[r]) at out + r out_stride, out_cap_frames items of room per row.  *n_frames =
 * floor((carried + n_in) / M) items are written to every row.  More than max_frames M samples or
 * fewer than *n_frames items of room (GR4PM_ERR_OVERFLOW) are refused before anything is written. */
gr4pm_status gr4pm_channelizer_process(gr4pm_channelizer* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out,
                                       size_t out_stride, size_t out_cap_frames, size_t* n_frames);
/* in: DEVICE, n_in items of an integer IQ format (gr4pm_iq_format below; scale 0: the format's default).
 * The same contract as gr4pm_channelizer_process, and its result on gr4pm_iq_unpack(in) bit for bit: the
 * samples are converted where they enter the kernel, the handle's history stays complex64, so calls of
 * any format may be mixed on one handle. */
gr4pm_status gr4pm_channelizer_process_iq(gr4pm_channelizer* h, const void* in, int format, float scale, size_t n_in,
                                          gr4pm_c64* out, size_t out_stride, size_t out_cap_frames, size_t* n_frames);

/* ====================================================================================
 * Ddc -- tunable down-converter: K frequency-translating decimating FIRs over one wideband c64 stream
 * (the project's own block: the reference is a one-channel modem).  Any integer decimation D in
 * [1, 1024], K in [1, 64] channels at arbitrary frequencies, a real prototype h[0 .. L - 1] with
 * 1 <= L <= 8192 (L need not be a multiple of D).  Output: channel-major at fs / D, in the layout
 * gr4pm_multichannel_receiver_submit takes.  With x[i] = 0 before the handle's first sample, whose
 * absolute index is start_index:
 *     w_k = llrint(f_k 2^32) mod 2^32 (uint32: the resolution is fs / 2^32)
 *     phi_k(i) = (w_k i) mod 2^32, in wrapping unsigned arithmetic: exact at any stream position,
 *                never accumulated in floating point
 *     y_k[n] = sum_{t = 0}^{L - 1} h[t] x[i - t] exp(-2 pi j phi_k(i - t) / 2^32),  i = start_index + n D + D - 1
 * (the D - 1 is the channelizer's w_k[n M + M - 1]: with D = M, f_k = k / M and the same taps this is the
 * channelizer's row k).  Evaluated as
 *     g_k[t] = h[t] exp(+2 pi j phi_k(t) / 2^32)   made at create on the host in double, each component
 *                                                  rounded to float once
 *     r_k[n] = exp(-2 pi j phi_k(i) / 2^32)        on the device: double sincospi of -phi / 2^31 (exact
 *                                                  argument), each component rounded to float
 *     y_k[n] = r_k[n] sum_t g_k[t] x[i - t]
 * with one complex accumulator per channel, t ascending, every complex multiply-accumulate four fmaf:
 *     re = fmaf(gr, xr, re); re = fmaf(-gi, xi, re); im = fmaf(gr, xi, im); im = fmaf(gi, xr, im)
 * and the product with r_k[n] the same four fmaf from zero.  A result is a function of (k, n, stream)
 * only: it does not depend on how the stream is cut into calls.  The last L - 1 samples and the
 * samples of an incomplete frame stay in the handle on the device as complex64; the absolute index
 * lives on the host.  process() takes any n_in, enqueues on the handle's stream and does not wait.
 * Frequencies are fixed at create.
 * ================================================================================== */
typedef struct gr4pm_ddc gr4pm_ddc;
typedef struct {
    size_t n_channels;          /* K: 1 .. 64 */
    size_t decimation;          /* D: 1 .. 1024 */
    const double* frequencies;  /* host: K frequencies in cycles per input sample, any finite value */
    const float* taps;          /* host: n_taps prototype taps, copied at create (NULL: the default design,
                                   gr4pm_ddc_taps(D, 12, 0.25, 0.75)) */
    size_t n_taps;              /* L: 1 .. 8192 (ignored when taps is NULL) */
    size_t max_frames;          /* per process() call: n_in <= max_frames D; 1..2^31 */
    uint64_t start_index;       /* absolute index of the first sample the handle sees */
    void* stream;               /* hipStream_t (NULL: the default stream) */
} gr4pm_ddc_params;
/* The Kaiser design of gr4pm_channelizer_taps with L = taps_per_phase * decimation taps, for any integer
 * decimation (host only).  passband / stopband: the band edges in units of the output rate fs / D;
 * DC gain 1.  For a power-of-two decimation the floats are those of gr4pm_channelizer_taps.
 * out: taps_per_phase * decimation floats. */
gr4pm_status gr4pm_ddc_taps(size_t decimation, size_t taps_per_phase, double passband, double stopband, float* out);
gr4pm_status gr4pm_ddc_create(const gr4pm_ddc_params* params, gr4pm_ddc** out);
void gr4pm_ddc_destroy(gr4pm_ddc* h);
/* back to start_index with zero history and no carried samples */
gr4pm_status gr4pm_ddc_reset(gr4pm_ddc* h);
/* frames the next process() of n_in samples produces (from lengths, on the host); the state is unchanged */
gr4pm_status gr4pm_ddc_output_items(const gr4pm_ddc* h, size_t n_in, size_t* n_frames);
/* out: K doubles (host), the quantised frequencies w_k / 2^32 folded to [-0.5, 0.5) */
gr4pm_status gr4pm_ddc_frequencies(const gr4pm_ddc* h, double* out);
/* in: DEVICE, n_in samples (any number; all are consumed).  out: DEVICE, channel k at out + k out_stride,
 * out_cap_frames items of room per row.  *n_frames = floor((carried + n_in) / D) items are written to
 * every row.  A refused call -- a NULL pointer, out_stride < *n_frames with K > 1 (GR4PM_ERR_INVALID),
 * more than max_frames D samples or fewer than *n_frames items of room (GR4PM_ERR_OVERFLOW) -- sets
 * gr4pm_last_error and *n_frames = 0, writes nothing and does not move the stream. */
gr4pm_status gr4pm_ddc_process(gr4pm_ddc* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_stride,
                               size_t out_cap_frames, size_t* n_frames);
/* in: DEVICE, n_in items of an integer IQ format (gr4pm_iq_format below; scale 0: the format's default).
 * The same contract as gr4pm_ddc_process, and its result on gr4pm_iq_unpack(in) bit for bit: the samples
 * are converted where they enter the kernel, the handle's history stays complex64, so calls of any format
 * may be mixed on one handle. */
gr4pm_status gr4pm_ddc_process_iq(gr4pm_ddc* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                  size_t out_stride, size_t out_cap_frames, size_t* n_frames);

/* ------------------------------------------------------------------------------------
 * Ddc, rational resampling by I / D (output rate fs I / D) in the same pass: a gr4pm_ddc handle made by
 * gr4pm_ddc_create_rational.  I in [1, 64], D in [1, 1024], gcd(I, D) = 1 (a pair
 * that is not in lowest terms is refused with GR4PM_ERR_INVALID, the message names the reduced pair).
 * The real prototype h[0 .. L - 1], 1 <= L <= 8192, runs at the virtual rate I fs; L need not be a
 * multiple of I: P = ceil(L / I) and h[t] = 0 for t >= L.  w_k, phi_k and x = 0 before the handle's
 * first sample are the Ddc's above.  Output item n, counted from the handle's start:
 *     m_n = n D + D - 1                  its index in the stream zero-stuffed by I
 *     i_n = start_index + m_n div I      its input index
 *     p_n = m_n mod I                    its polyphase branch
 *     y_k[n] = sum_{s = 0}^{P - 1} h[p_n + s I] x[i_n - s] exp(-2 pi j phi_k(i_n - s) / 2^32)
 * With I = 1 this is the Ddc item for item.  For a fixed branch p the items n, n + I, n + 2 I, ... have
 * i stepping by exactly D: every branch is an integer-D Ddc with the taps h[p::I].  Evaluated as
 *     g_k[p][s] = h[p + s I] exp(+2 pi j phi_k(s) / 2^32)   on the host in double, with the Ddc's quadrant
 *                                                           reduction, each component rounded to float once
 *     r_k[n] = exp(-2 pi j phi_k(i_n) / 2^32)               double sincospi of the exact argument, rounded
 *     y_k[n] = r_k[n] sum_s g_k[p_n][s] x[i_n - s]
 * with one accumulator per channel, s ascending over the taps of h[p_n::I], every complex
 * multiply-accumulate the Ddc's four fmaf in its order and the product with r_k[n] the same four from
 * zero.  A result is a function of (k, n, stream) only: not of the call cuts, the grid or the input's format.
 * Stream contract: all input of a call is consumed; item n exists as soon as sample i_n has arrived, so
 * after N samples in all floor(N I / D) items exist per row.  The handle keeps P - 1 samples of history
 * on the device and never a partial frame; the position (the next item's input index and branch, and the
 * samples taken) lives on the host in 64-bit integers and reaches the kernel by value; process() reads
 * nothing back.  With I > D a call makes more items than it takes samples: max_frames bounds the
 * output items of a call, n_in I <= max_frames D.
 * gr4pm_ddc_process / _process_iq / _reset / _output_items / _frequencies / _destroy take such a handle
 * with the contracts documented above; *n_frames is the item count of this section.  interpolation = 1
 * makes the handle gr4pm_ddc_create makes, with its results bit for bit.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    size_t n_channels;          /* K: 1 .. 64 */
    size_t decimation;          /* D: 1 .. 1024 */
    const double* frequencies;  /* host: K frequencies in cycles per input sample, any finite value */
    const float* taps;          /* host: n_taps prototype taps at the rate I fs, copied at create (NULL: the default
                                   design, gr4pm_ddc_rational_taps(I, D, 12, 0.25, 0.75)) */
    size_t n_taps;              /* L: 1 .. 8192 (ignored when taps is NULL) */
    size_t max_frames;          /* output items per process() call: n_in I <= max_frames D; 1..2^31 */
    uint64_t start_index;       /* absolute index of the first sample the handle sees */
    void* stream;               /* hipStream_t (NULL: the default stream) */
    size_t interpolation;       /* I: 1 .. 64, gcd(I, D) = 1 */
} gr4pm_ddc_rational_params;
/* The Kaiser design of gr4pm_ddc_taps with L = taps_per_phase * decimation taps at the virtual rate I fs
 * (the span of gr4pm_ddc_taps in output items) and DC gain I (every polyphase branch has gain about 1),
 * scaled in double before the one rounding to float (host only).  passband / stopband: the band edges in
 * units of the output rate fs I / D; refused when the cutoff, midway between them, exceeds half of the
 * lower of the input and the output rate: passband + stopband <= min(1, D / I).  With I = 1 the floats
 * are those of gr4pm_ddc_taps.  out: taps_per_phase * decimation floats. */
gr4pm_status gr4pm_ddc_rational_taps(size_t interpolation, size_t decimation, size_t taps_per_phase, double passband,
                                     double stopband, float* out);
gr4pm_status gr4pm_ddc_create_rational(const gr4pm_ddc_rational_params* params, gr4pm_ddc** out);

/* ------------------------------------------------------------------------------------
 * Ddc, burst spans of a recording.  A Ddc item is a function of (k, n, stream) only,
 * so any stretch of any channel's output can be computed on its own: one call computes n_spans spans
 * (channel, first frame, frame count) of an integer-D handle's output, each into a row of its own, in
 * the [rows, n] layout gr4pm_multichannel_receiver_submit takes.
 *   in[0] is the stream's sample with the absolute index in_index.  For this call the stream is `in`
 *   inside [in_index, in_index + n_in) and zero everywhere else, including everything before the
 *   handle's start_index.  Frames are numbered as the streaming handle numbers them: frame n of channel
 *   k is y_k[n] above, with i = start_index + n D + D - 1, whatever the handle has processed so far.
 *     out[b out_stride + c] = y_{spans[b].channel}[spans[b].first_frame + c]   for c < spans[b].n_frames
 *     out[b out_stride + c] = +0                                               for n_frames <= c < n_cols
 *   so that `out` may be uninitialised and a row can go to a receiver as it is.  The evaluation is the
 *   streaming one (the handle's rotated-tap table and frequency words, one accumulator, t ascending, the
 *   same fmaf): a row has the bits of the streaming output's slice.
 * The call does not touch the handle's stream state: a process() after it gives what it would have
 * given without it.  It enqueues on the handle's stream, does not wait and reads nothing back.
 * Refused, with gr4pm_last_error set and nothing enqueued: a handle with interpolation > 1, more than 64
 * spans in a call, channel >= K, n_spans > 1 with out_stride < n_cols, a NULL spans / out / (with
 * n_in > 0) in, an invalid format (all GR4PM_ERR_INVALID); n_frames > n_cols, and a span or a buffer
 * whose last sample's index does not fit 64 bits: (first_frame + n_frames) D + max(start_index, L - 1)
 * > 2^64 - 2 or in_index + n_in > 2^64 - 1 (both GR4PM_ERR_OVERFLOW).  n_spans = 0 or n_cols = 0: OK, nothing done.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    uint32_t channel;     /* < K */
    uint32_t n_frames;    /* <= n_cols; 0: the row is all zeros */
    uint64_t first_frame; /* counted from the handle's start_index */
} gr4pm_ddc_span;
/* in: DEVICE, n_in samples.  spans: HOST, n_spans items (copied by the call).  out: DEVICE, n_spans rows. */
gr4pm_status gr4pm_ddc_extract(gr4pm_ddc* h, const gr4pm_c64* in, size_t n_in, uint64_t in_index, const gr4pm_ddc_span* spans,
                               size_t n_spans, gr4pm_c64* out, size_t out_stride, size_t n_cols);
/* in: DEVICE, n_in items of an integer IQ format (scale 0: the format's default), converted where the
 * kernel loads them: the result of gr4pm_ddc_extract on gr4pm_iq_unpack(in), bit for bit. */
gr4pm_status gr4pm_ddc_extract_iq(gr4pm_ddc* h, const void* in, int format, float scale, size_t n_in, uint64_t in_index,
                                  const gr4pm_ddc_span* spans, size_t n_spans, gr4pm_c64* out, size_t out_stride,
                                  size_t n_cols);

/* ====================================================================================
 * Duc -- tunable up-converter, the mirror of the Ddc: K complex64 rows at fs / I become ONE wideband
 * stream at fs (the project's own block).  Any integer interpolation I in [1, 1024], K in [1, 64] rows
 * at arbitrary frequencies, a real prototype h[0 .. L - 1] with 1 <= L <= 8192 (L need not be a multiple
 * of I; P = ceil(L / I)), real gains a_k.  With v_k[m] = 0 before the handle's first item, output sample
 * j = m I + r (0 <= r < I) at the absolute index i = start_index + j:
 *     w_k = llrint(f_k 2^32) mod 2^32,  phi_k(i) = (w_k i) mod 2^32   (as in the Ddc: wrapping unsigned
 *                                                                       arithmetic, exact anywhere)
 *     x[i] = sum_k a_k exp(+2 pi j phi_k(i) / 2^32) sum_{p : p I + r < L} h[p I + r] v_k[m - p]
 * (zero-stuff every row by I, filter with h, mix to f_k, sum).  Evaluated as
 *     g_k[t] = a_k h[t] exp(+2 pi j phi_k(t) / 2^32)   made at create on the host in double (the Ddc's table
 *                                                      times a_k), each component rounded to float once
 *     q_k[m'] = exp(+2 pi j phi_k(start_index + m' I) / 2^32)   one per INPUT item, on the device: double
 *                                                      sincospi of phi / 2^31 (exact argument), each
 *                                                      component rounded to float
 *     z_k[m'] = q_k[m'] v_k[m']                        four fmaf from zero
 *     x[i] = sum_k sum_{p : p I + r < L} g_k[p I + r] z_k[m - p]
 * with ONE complex accumulator per output sample that starts at zero, k ascending in the outer loop,
 * p ascending in the inner one, every complex multiply-accumulate the Ddc's four fmaf:
 *     re = fmaf(gr, zr, re); re = fmaf(-gi, zi, re); im = fmaf(gr, zi, im); im = fmaf(gi, zr, im)
 * A result is a function of (absolute output index, the rows' streams) only: it does not depend on how
 * the streams are cut into calls.  A call of n_in items per row writes exactly n_in I samples; the last
 * P - 1 items of every row stay in the handle on the device, the absolute index lives on the host.
 * process() enqueues on the handle's stream and does not wait.  Frequencies and gains are fixed at create.
 * ================================================================================== */
typedef struct gr4pm_duc gr4pm_duc;
typedef struct {
    size_t n_channels;          /* K: 1 .. 64 */
    size_t interpolation;       /* I: 1 .. 1024 */
    const double* frequencies;  /* host: K frequencies in cycles per output sample, any finite value */
    const double* gains;        /* host: K finite real gains a_k (NULL: all 1) */
    const float* taps;          /* host: n_taps prototype taps, copied at create (NULL: the default design,
                                   gr4pm_duc_taps(I, 12, 0.25, 0.75)) */
    size_t n_taps;              /* L: 1 .. 8192 (ignored when taps is NULL) */
    size_t max_items;           /* per process() call: n_in <= max_items; 1..2^31 */
    uint64_t start_index;       /* absolute index of the first output sample */
    void* stream;               /* hipStream_t (NULL: the default stream) */
} gr4pm_duc_params;
/* The Kaiser design of gr4pm_ddc_taps with L = taps_per_phase * interpolation taps and DC gain I (every
 * polyphase branch has gain about 1), scaled in double before the one rounding to float (host only).
 * passband / stopband: the band edges in units of the input rate fs / I.
 * out: taps_per_phase * interpolation floats. */
gr4pm_status gr4pm_duc_taps(size_t interpolation, size_t taps_per_phase, double passband, double stopband, float* out);
gr4pm_status gr4pm_duc_create(const gr4pm_duc_params* params, gr4pm_duc** out);
void gr4pm_duc_destroy(gr4pm_duc* h);
/* back to start_index with zero history */
gr4pm_status gr4pm_duc_reset(gr4pm_duc* h);
/* samples the next process() of n_in items per row produces: n_in I; the state is unchanged */
gr4pm_status gr4pm_duc_output_items(const gr4pm_duc* h, size_t n_in, size_t* n_out);
/* out: K doubles (host), the quantised frequencies w_k / 2^32 folded to [-0.5, 0.5) */
gr4pm_status gr4pm_duc_frequencies(const gr4pm_duc* h, double* out);
/* the consecutive output samples one workgroup of the handle's kernel owns (its tile): what a test needs to know to cut
 * a call across a tile's end; no result depends on it */
gr4pm_status gr4pm_duc_tile_items(const gr4pm_duc* h, size_t* samples);
/* in: DEVICE, row k at in + k in_stride, n_in items each (any number).  out: DEVICE, contiguous, out_cap
 * samples of room; *n_out = n_in I samples are written.  A refused call -- a NULL pointer, in_stride < n_in
 * with K > 1 (GR4PM_ERR_INVALID), more than max_items items or fewer than n_in I samples of room
 * (GR4PM_ERR_OVERFLOW) -- sets gr4pm_last_error and *n_out = 0, writes nothing and does not move the
 * stream. */
gr4pm_status gr4pm_duc_process(gr4pm_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, gr4pm_c64* out,
                               size_t out_cap, size_t* n_out);
/* The same call with the samples written as integer IQ (gr4pm_iq_format, below): out is
 * DEVICE memory in ITEMS of `format` (2 or 4 bytes, aligned to the item only), out_cap counts items, gain 0 is
 * the format's default, clipped is NULL or a DEVICE counter the call ADDS to.  The bytes and the count are
 * gr4pm_iq_pack's of what gr4pm_duc_process would have written: the kernel packs each sample where it holds it
 * and has no complex64 store.  Serves rational handles too.  The handle's state stays complex64: calls of any
 * format mix on one handle.  An unknown format (GR4PM_ERR_INVALID) and everything gr4pm_duc_process refuses,
 * with its status, are refused before anything is enqueued: gr4pm_last_error set, *n_out = 0, the stream not
 * moved. */
gr4pm_status gr4pm_duc_process_iq(gr4pm_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, void* out, int format,
                                  float gain, size_t out_cap, size_t* n_out, unsigned long long* clipped);

/* ------------------------------------------------------------------------------------
 * Duc, rational resampling by I / D (output rate fs_in I / D) in the same pass: a gr4pm_duc handle made by
 * gr4pm_duc_create_rational, the mirror of gr4pm_ddc_create_rational.  I in
 * [1, 1024], D in [1, 64], gcd(I, D) = 1 (a pair that is not in lowest terms is refused with
 * GR4PM_ERR_INVALID, the message names the reduced pair).  The real prototype h[0 .. L - 1], 1 <= L <= 8192,
 * runs at the virtual rate I fs_in; P = ceil(L / I) and h[t] = 0 for t >= L.  w_k, phi_k, the gains a_k and
 * v_k[m] = 0 before the handle's first item are the Duc's above.  Output sample j, counted from the
 * handle's start:
 *     i   = start_index + j      its absolute index (uint64)
 *     u_j = j D                  its index in the rows zero-stuffed by I
 *     m_j = u_j div I            its newest item
 *     r_j = u_j mod I            its polyphase branch
 *     x[i] = sum_k a_k exp(+2 pi j phi_k(i) / 2^32) sum_{p : p I + r_j < L} h[p I + r_j] v_k[m_j - p]
 * (zero-stuff every row by I, filter with h at the rate I fs_in, keep every D-th, mix, sum).  With D = 1
 * this is the Duc sample for sample.  j and m_j - p are not an integer apart, so there is no rotator per
 * input item: filter first, then mix.  Evaluated as
 *     g_k[t] = fl(a_k h[t])                                   the product in double, rounded to float once
 *     b_k[j] = sum_{p : p I + r_j < L} g_k[p I + r_j] v_k[m_j - p]
 *                                                             from zero, p ascending, per step
 *                                                             re = fmaf(g, vr, re); im = fmaf(g, vi, im)
 *     q_k(i) = A_k[i div B] (x) T_k[i mod B],  B = 1024       A_k[n]: double sincospi of phi_k(n B) / 2^31 (exact
 *                                                             argument) on the device, rounded to float;
 *                                                             T_k[t] = exp(+2 pi j phi_k(t) / 2^32) made at create
 *                                                             on the host in double with the Ddc's quadrant
 *                                                             reduction, rounded to float; (x): the four fmaf of
 *                                                             the Ddc's multiply-accumulate from zero, A first
 *     x[i] = sum_k q_k(i) b_k[j]                              one accumulator from zero, k ascending, the same
 *                                                             four fmaf with q_k first
 * The rotator is aligned to the ABSOLUTE index, so a sample is a function of (absolute output index, the
 * rows' streams) only: not of the call cuts or the grid.
 * Stream contract: all input of a call is consumed; sample j exists once item m_j has arrived, so after N
 * items per row in all ceil(N I / D) samples exist, and a call writes the difference of that count across
 * the call: none is possible when I < D, several per item when I > D.  The handle keeps P - 1 items of
 * every row on the device; the position (items taken, the next sample's m and r) lives on the host in
 * 64-bit integers, advanced by (r + F D) divmod I after a call of F samples, and reaches the kernel by
 * value; process() reads nothing back.  max_items bounds n_in; out_cap must hold the call's samples.
 * gr4pm_duc_process / _reset / _output_items / _frequencies / _destroy take such a handle with the
 * contracts documented above; *n_out and output_items are the sample count of this section, which
 * depends on the handle's position.  decimation = 1 makes the handle gr4pm_duc_create makes, with its
 * results bit for bit.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    size_t n_channels;          /* K: 1 .. 64 */
    size_t interpolation;       /* I: 1 .. 1024 */
    const double* frequencies;  /* host: K frequencies in cycles per output sample, any finite value */
    const double* gains;        /* host: K finite real gains a_k (NULL: all 1) */
    const float* taps;          /* host: n_taps prototype taps at the rate I fs_in, copied at create (NULL: the default
                                   design, gr4pm_duc_rational_taps(I, D, 12, 0.25, 0.75), which exists for I >= D) */
    size_t n_taps;              /* L: 1 .. 8192 (ignored when taps is NULL) */
    size_t max_items;           /* per process() call: n_in <= max_items; 1..2^31 */
    uint64_t start_index;       /* absolute index of the first output sample */
    void* stream;               /* hipStream_t (NULL: the default stream) */
    size_t decimation;          /* D: 1 .. 64, gcd(I, D) = 1 */
} gr4pm_duc_rational_params;
/* The Kaiser design of gr4pm_duc_taps with L = taps_per_phase * interpolation taps and DC gain I, scaled
 * in double before the one rounding to float (host only).  passband / stopband: the band edges in units
 * of the input rate; refused when the cutoff, midway between them, exceeds half of the lower of the input
 * and the output rate: passband + stopband <= min(1, I / D).  With D = 1 the floats are those of
 * gr4pm_duc_taps.  out: taps_per_phase * interpolation floats. */
gr4pm_status gr4pm_duc_rational_taps(size_t interpolation, size_t decimation, size_t taps_per_phase, double passband,
                                     double stopband, float* out);
gr4pm_status gr4pm_duc_create_rational(const gr4pm_duc_rational_params* params, gr4pm_duc** out);

/* ====================================================================================
 * Integer IQ formats (the project's own block: the reference moves complex64 only).  An item is one
 * complex sample, I then Q, little-endian integers.
 *     format          item         unpack, per component            default scale   default gain
 *     GR4PM_IQ_SC16   2 x int16    float(v) * scale                 2^-15           2^15
 *     GR4PM_IQ_SC8    2 x int8     float(v) * scale                 2^-7            2^7
 *     GR4PM_IQ_CU8    2 x uint8    (float(v) - 127.5f) * scale      2^-7            2^7
 * Every float operation rounds on its own; the conversion and the offset are exact, so unpack is one
 * rounding.  pack, per component: t = x * gain (cu8: then t = t + 127.5f), r = rintf(t) (ties to even),
 * r clamped to the type's range; NaN gives 0 (cu8: 128).  A component that was clamped or was NaN counts
 * as clipped.  A scale or gain of 0 means the default.
 * ================================================================================== */
typedef enum {
    GR4PM_IQ_SC16 = 1,
    GR4PM_IQ_SC8 = 2,
    GR4PM_IQ_CU8 = 3
} gr4pm_iq_format;
/* in, out: DEVICE, `rows` rows of n items at strides (in items) of in_stride and out_stride; rows == 1 is
 * the plain stream, [rows][stride] the multi-channel receiver's layout.  Pointers need the alignment of
 * their item only (2 or 4 bytes; 8 for complex64).  in and out must not overlap (not checked).
 * Stateless: enqueues on `stream` (hipStream_t, NULL: the default stream) and does not wait.  An unknown
 * format, a NULL pointer with n > 0 or a stride below n (GR4PM_ERR_INVALID) are refused before any HIP
 * call. */
gr4pm_status gr4pm_iq_unpack(const void* in, size_t in_stride, int format, float scale, size_t rows, size_t n,
                             gr4pm_c64* out, size_t out_stride, void* stream);
/* clipped: NULL, or a DEVICE counter the call ADDS the number of clipped components to (one atomic per
 * workgroup that clipped anything). */
gr4pm_status gr4pm_iq_pack(const gr4pm_c64* in, size_t in_stride, size_t rows, size_t n, int format, float gain,
                           void* out, size_t out_stride, unsigned long long* clipped, void* stream);

/* ====================================================================================
 * Spectrum -- Welch power spectral density of one wideband stream on the device, and a carrier finder
 * made from it (the project's own block).  The stream is x[0], x[1], ... over all
 * calls since create or reset; N = fft_size = 2048, 1 <= hop <= N:
 *     segment s        x[s hop .. s hop + N); no zero prehistory: after T samples there are
 *                      T < N ? 0 : (T - N) / hop + 1 segments
 *     X_s            = FFT_N(w . x_s)     forward sign, unnormalised, FFT bin order (bin k: +k / N cycles
 *                                         per sample, k > N / 2: negative frequencies)
 *     acc[k]         = sum_s |X_s[k]|^2
 *     mean[k]        = acc[k] / (segments sum_n w[n]^2)
 *     max_hold[k]    = max_s |X_s[k]|^2 / sum_n w[n]^2
 * so white noise with E|x|^2 = sigma^2 reads sigma^2 in every bin of mean.  A wave transforms a run of at
 * most gr4pm_spectrum_float_run() consecutive segments and sums their powers in float32; the runs' sums
 * are added in double, in stream order, with no floating-point atomic: the same calls give the same
 * bits.  max_hold does not depend on how the stream is cut into calls at all.  process() takes any n,
 * consumes all of it, enqueues on the handle's stream and does not wait; the samples of the segment that
 * is not complete yet (fewer than N) stay on the device as complex64.
 * ================================================================================== */
typedef struct gr4pm_spectrum gr4pm_spectrum;
typedef struct {
    uint32_t fft_size;          /* N: 2048 */
    uint32_t hop;               /* 1 .. N */
    const float* window;        /* host: N floats, copied at create (NULL: the periodic Hann window) */
    void* stream;               /* hipStream_t (NULL: the default stream) */
} gr4pm_spectrum_params;
/* the periodic Hann window 0.5 - 0.5 cos(2 pi i / n), computed in double and rounded to float once (host only) */
gr4pm_status gr4pm_spectrum_window(uint32_t n, float* out);
/* segments a wave sums in float32 before its sum goes on in double: 64 */
uint32_t gr4pm_spectrum_float_run(void);
/* fft_size != 2048, hop == 0, hop > N or a window with a non-finite value: GR4PM_ERR_INVALID, no handle */
gr4pm_status gr4pm_spectrum_create(const gr4pm_spectrum_params* params, gr4pm_spectrum** out);
void gr4pm_spectrum_destroy(gr4pm_spectrum* h);
/* back to the fresh stream: no segments, no carried samples */
gr4pm_status gr4pm_spectrum_reset(gr4pm_spectrum* h);
/* x: DEVICE, n complex64 samples (any number, 0 and 1 included; all are consumed) */
gr4pm_status gr4pm_spectrum_process(gr4pm_spectrum* h, const void* x, size_t n);
/* x: DEVICE, n items of an integer IQ format (gr4pm_iq_format; scale 0: the format's default).  The result of
 * gr4pm_spectrum_process on gr4pm_iq_unpack(x) bit for bit: the samples are converted where the kernel loads
 * them, the carried samples stay complex64, so calls of any format may be mixed on one handle. */
gr4pm_status gr4pm_spectrum_process_iq(gr4pm_spectrum* h, const void* x, int format, float scale, size_t n);
/* mean: N doubles, max_hold: N floats (host; either may be NULL), *segments: the count (may be NULL).  Waits
 * for the handle's stream; the divisions happen in double on the host.  With no segment yet: zeros. */
gr4pm_status gr4pm_spectrum_read(gr4pm_spectrum* h, double* mean, float* max_hold, uint64_t* segments);

/* Carriers from a power spectrum of n bins in FFT order, host only.  floor: the lower median, element
 * (n - 1) / 2 of the sorted bins.  A bin is occupied when it exceeds floor 10^(threshold_db / 10).  Runs of
 * occupied bins are taken on the circle of n bins (a carrier across +-0.5 is one run); runs separated by at
 * most max_gap_bins free bins merge, then runs shorter than min_width_bins are dropped.  Per run of n_bins
 * bins from first_bin, over i = 0 .. n_bins - 1 in double, in index order:
 *     c = sum i (psd - floor) / sum (psd - floor),  frequency = (first_bin + c) / n folded to [-0.5, 0.5),
 *     bandwidth = n_bins / n,  power = sum (psd - floor),  snr_db = 10 log10(peak / floor)
 * out: room for cap carriers; the first min(cap, *count) in ascending frequency are written, *count is the
 * number found.  n == 0, a NULL psd or count, or threshold_db <= 0 (or NaN): GR4PM_ERR_INVALID. */
typedef struct {
    double threshold_db;        /* > 0 */
    size_t max_gap_bins;
    size_t min_width_bins;
} gr4pm_carrier_params;
typedef struct {
    double frequency;           /* cycles per sample, [-0.5, 0.5) */
    double bandwidth;           /* cycles per sample */
    double power;               /* above the floor, summed over the run */
    double snr_db;
    uint64_t first_bin;
    uint64_t n_bins;
} gr4pm_carrier;
gr4pm_status gr4pm_find_carriers(const double* psd, size_t n, const gr4pm_carrier_params* params, gr4pm_carrier* out,
                                 size_t cap, size_t* count);

/* ====================================================================================
 * Spectrogram -- PSD rows over time of one wideband stream on the device, the power of bands of those rows,
 * and a burst finder made from it (the project's own block).  Segments and X_s are
 * exactly the Spectrum's above (N = fft_size = 2048, 1 <= hop <= N, no zero prehistory).  With
 * R = average, 1 <= R <= gr4pm_spectrum_float_run() (64):
 *     row t            is made of the segments t R .. t R + R - 1 and exists once segment t R + R - 1 is
 *                      complete: after S segments there are S / R rows.  Row t covers the samples
 *                      [t R hop, t R hop + (R - 1) hop + N).
 *     mean detector    row[t][k] = fl32( (sum_s |X_s[k]|^2) inv ),  inv = fl32(1 / (R sum_n w[n]^2));
 *                      the sum in float32, in segment order, starting from the first power itself
 *     max detector     row[t][k] = fl32( (max_s |X_s[k]|^2) inv ),  inv = fl32(1 / sum_n w[n]^2)
 * inv is computed in double on the host and rounded once; the product at the store is the only one.  White
 * noise with E|x|^2 = sigma^2 reads sigma^2 in every bin of a mean row.  Between calls the handle keeps the
 * samples of the incomplete segment, as the Spectrum does, and the incomplete row: 2048 float32 sums or
 * maxima on the device and the count S mod R.  A row that goes on from them adds or maximises the same
 * values in the same order, so THE ROWS DO NOT DEPEND ON HOW THE STREAM IS CUT INTO CALLS, BIT FOR BIT.
 * ================================================================================== */
typedef struct gr4pm_spectrogram gr4pm_spectrogram;
enum { GR4PM_SPECTROGRAM_MEAN = 0, GR4PM_SPECTROGRAM_MAX = 1 };
typedef struct {
    uint32_t fft_size;          /* N: 2048 */
    uint32_t hop;               /* 1 .. N */
    uint32_t average;           /* R: segments per row, 1 .. gr4pm_spectrum_float_run() */
    uint32_t detector;          /* GR4PM_SPECTROGRAM_MEAN or GR4PM_SPECTROGRAM_MAX */
    const float* window;        /* host: N floats, copied at create (NULL: the periodic Hann window) */
    void* stream;               /* hipStream_t (NULL: the default stream) */
} gr4pm_spectrogram_params;
/* fft_size != 2048, hop == 0, hop > N, a window with a non-finite value, average == 0, average > 64 or an
 * unknown detector: GR4PM_ERR_INVALID, no handle */
gr4pm_status gr4pm_spectrogram_create(const gr4pm_spectrogram_params* params, gr4pm_spectrogram** out);
void gr4pm_spectrogram_destroy(gr4pm_spectrogram* h);
/* back to the fresh stream: no segments, no carried samples, no carried row */
gr4pm_status gr4pm_spectrogram_reset(gr4pm_spectrogram* h);
/* *rows: the rows a call of n samples would complete now */
gr4pm_status gr4pm_spectrogram_rows(const gr4pm_spectrogram* h, size_t n, size_t* rows);
/* x: DEVICE, n complex64 samples (any number, 0 included; all are consumed).  rows: DEVICE, room for rows_cap
 * rows of N floats; the call writes the *n_rows rows it completes (gr4pm_spectrogram_rows' count), in FFT bin
 * order.  Enqueues on the handle's stream and does not wait.  rows_cap below that count: GR4PM_ERR_OVERFLOW,
 * and the handle is as it was.  n_rows may be NULL. */
gr4pm_status gr4pm_spectrogram_process(gr4pm_spectrogram* h, const void* x, size_t n, float* rows, size_t rows_cap,
                                       size_t* n_rows);
/* x: DEVICE, n items of an integer IQ format (gr4pm_iq_format; scale 0: the format's default).  The result of
 * gr4pm_spectrogram_process on gr4pm_iq_unpack(x) bit for bit; calls of any format may be mixed on one handle. */
gr4pm_status gr4pm_spectrogram_process_iq(gr4pm_spectrogram* h, const void* x, int format, float scale, size_t n,
                                          float* rows, size_t rows_cap, size_t* n_rows);
/* The power of bands of rows.  rows: DEVICE, n_rows rows of N floats (what process wrote, or any such array).
 * bands: HOST, n_bands <= 64 bands of the bins first_bin .. first_bin + n_bins - 1 mod N (first_bin < N,
 * 1 <= n_bins <= N: a band across +-0.5 is one band).  out: DEVICE, double out[n_bands][n_rows]: the sum of the
 * band's bins of each row, in double.  One wave per row adds in a fixed order and there is no atomic: the same
 * call gives the same bits.  Enqueues on the handle's stream and does not wait. */
typedef struct {
    uint32_t first_bin;
    uint32_t n_bins;
} gr4pm_band;
gr4pm_status gr4pm_spectrogram_band_power(gr4pm_spectrogram* h, const float* rows, size_t n_rows, const gr4pm_band* bands,
                                          size_t n_bands, double* out);

/* Bursts from a band's power over time, n rows in time order, host only.  floor: params->floor if > 0, else the
 * lower median, element (n - 1) / 2 of the sorted rows.  A row is active when it exceeds
 * floor 10^(threshold_db / 10).  Runs of active rows are taken in time order (nothing wraps); runs separated by
 * at most max_gap_rows inactive rows merge, then runs shorter than min_rows are dropped (the length counts the
 * bridged rows).  Per run of n_rows rows from first_row, in double, in index order:
 *     power = the mean of (p - floor),  peak_row = the first row of the maximum,  snr_db = 10 log10(peak / floor)
 * out: room for cap bursts; the first min(cap, *count) in ascending time are written, *count is the number
 * found.  n == 0, a NULL power, params or count, threshold_db <= 0 (or NaN), a negative or non-finite floor:
 * GR4PM_ERR_INVALID. */
typedef struct {
    double threshold_db;        /* > 0 */
    double floor;               /* > 0: the noise level of a row; 0: the lower median of the rows */
    size_t max_gap_rows;
    size_t min_rows;
} gr4pm_burst_params;
typedef struct {
    uint64_t first_row;
    uint64_t n_rows;
    uint64_t peak_row;
    double power;               /* above the floor, the mean over the run */
    double snr_db;
} gr4pm_burst;
gr4pm_status gr4pm_find_bursts(const double* power, size_t n, const gr4pm_burst_params* params, gr4pm_burst* out,
                               size_t cap, size_t* count);

/* ====================================================================================
 * LineSpectrum -- the Welch spectrum of a memoryless nonlinearity of rows of channel items, whose spectral
 * line gives a burst's residual carrier offset (x^4, x^2) or its symbol rate (|x|^2); a line finder and a
 * rational approximation made for it (the project's own block).  N = fft_size = 2048,
 * 1 <= hop <= N, the window as gr4pm_spectrum_params'.  One call takes R <= 64 rows x[r stride + i] of a DEVICE
 * complex64 array (what gr4pm_ddc_extract or gr4pm_ddc_process wrote).  For row r with n_r = lengths[r] items
 * and u[i] = gains[r] x[r, i] (one float32 product per component):
 *     y[i]           = |u[i]|^2 (GR4PM_LINE_ENVELOPE, real), u[i]^2 (GR4PM_LINE_SQUARE) or (u[i]^2)^2
 *                      (GR4PM_LINE_FOURTH) for i < n_r, and 0 for i >= n_r.  ITEMS AT OR BEYOND n_r ARE NEVER
 *                      LOADED: a row may end at its buffer's last byte and may hold anything behind n_r.
 *     segments       S_r = 0 if n_r = 0, else 1 + ceil(max(n_r - N, 0) / hop); segment s is y[s hop .. s hop + N),
 *                      so the last one is zero-filled and a burst shorter than N items still has one
 *     square, fourth acc[k] = sum_s |FFT_N(w y_s)[k]|^2
 *     envelope       Z_p = FFT_N(w (y_2p + i y_2p+1)), an odd last segment pairs with zero;
 *                      acc[k] = sum_p (|Z_p[k]|^2 + |Z_p[(N - k) mod N]|^2) / 2, which is sum_s |Y_s[k]|^2 because y
 *                      is real; the fold happens in double, so the row is bit-symmetric in k <-> N - k
 *     out[r][k]      = acc[k] / (S_r sum_n w[n]^2), zeros when S_r = 0; FFT bin order (bin k: +k / N cycles per item)
 * A wave transforms a run of at most gr4pm_line_spectrum_float_run() (64) consecutive transforms of ONE row and
 * sums their powers in float32; the run length is fixed, and a row's runs are added in double, in order, with
 * no floating-point atomic: A ROW'S RESULT DEPENDS ON THAT ROW ALONE, BIT FOR BIT, not on the other rows of the
 * call or on R.  The kernel does not normalise: the powers are float32, so keep |gains[r] x| within about
 * 1e-4 .. 1e4 for GR4PM_LINE_FOURTH (1e-9 .. 1e9 for the other two); that is what `gains` is for.
 * ================================================================================== */
typedef struct gr4pm_line_spectrum gr4pm_line_spectrum;
enum { GR4PM_LINE_ENVELOPE = 0, GR4PM_LINE_SQUARE = 1, GR4PM_LINE_FOURTH = 2 };
typedef struct {
    uint32_t fft_size;          /* N: 2048 */
    uint32_t hop;               /* 1 .. N */
    const float* window;        /* host: N floats, copied at create (NULL: the periodic Hann window) */
    void* stream;               /* hipStream_t (NULL: the default stream) */
} gr4pm_line_spectrum_params;
/* transforms a wave sums in float32 before its sum goes on in double: 64 */
uint32_t gr4pm_line_spectrum_float_run(void);
/* fft_size != 2048, hop == 0, hop > N or a window with a non-finite value: GR4PM_ERR_INVALID, no handle */
gr4pm_status gr4pm_line_spectrum_create(const gr4pm_line_spectrum_params* params, gr4pm_line_spectrum** out);
void gr4pm_line_spectrum_destroy(gr4pm_line_spectrum* h);
/* x: DEVICE, R rows of n_cols items, `stride` items apart.  lengths: HOST, R items, copied by the call (NULL:
 * every row has n_cols items).  gains: DEVICE, R floats (NULL: 1).  out: DEVICE, double out[R][N].  Enqueues on
 * the handle's stream, does not wait and reads nothing back.  Refused with GR4PM_ERR_INVALID, gr4pm_last_error
 * set and nothing enqueued: R > 64, a length above n_cols, R > 1 with stride < n_cols, an unknown statistic, a
 * NULL x when any length is not zero, a NULL out; a row of more than 2^40 items: GR4PM_ERR_OVERFLOW.  R = 0: OK,
 * nothing done. */
gr4pm_status gr4pm_line_spectrum_process(gr4pm_line_spectrum* h, const gr4pm_c64* x, size_t stride, size_t n_cols,
                                         const uint64_t* lengths, size_t n_rows, const float* gains, int statistic,
                                         double* out);

/* The line of a spectrum of n bins in FFT order, host only.  The search window is the n_bins bins
 * (first_bin + i) mod n, i = 0 .. n_bins - 1, on the circle of n bins; first_bin < n,
 * 2 guard_bins + 3 <= n_bins <= n.
 *     peak        the first maximum in window order, at `bin`
 *     floor       the lower median of the window's bins: element (n_bins - 1) / 2 of them sorted
 *     snr_db    = 10 log10(peak / floor)
 *     margin_db = 10 log10(peak / other), other: the largest window bin whose circular distance to `bin` is
 *                 above guard_bins.  This is the confidence measure: the snr_db of pure noise grows with the
 *                 number of bins searched and shrinks with the segments averaged, margin_db stays near 0 dB.
 *     frequency = (bin + d) / n folded to [-0.5, 0.5), with the parabola through the natural logarithms of the
 *                 peak (lb) and its circular neighbours bin - 1 (la) and bin + 1 (lc), inside the window or not:
 *                 d = 0.5 (la - lc) / (la - 2 lb + lc), clamped to +-0.5; d = 0 if any of the three is <= 0 or the
 *                 curvature la - 2 lb + lc is not negative
 *     found     = peak > 0; without it frequency is the bin's and snr_db = margin_db = 0
 * n == 0, a NULL pointer, first_bin >= n, n_bins out of range: GR4PM_ERR_INVALID. */
typedef struct {
    uint64_t first_bin;
    uint64_t n_bins;
    uint64_t guard_bins;        /* the Python default is 2 */
} gr4pm_line_params;
typedef struct {
    double frequency;           /* cycles per item, [-0.5, 0.5) */
    double snr_db;
    double margin_db;
    double peak;
    double floor;
    uint64_t bin;
    uint64_t found;             /* 0 or 1 */
} gr4pm_line;
gr4pm_status gr4pm_find_line(const double* spectrum, size_t n, const gr4pm_line_params* params, gr4pm_line* out);

/* The fraction num / den with the smallest denominator (of several: the smallest numerator) inside
 * [value (1 - rel_tol), value (1 + rel_tol)], 1 <= num <= max_num, 1 <= den <= max_den, in lowest terms; host
 * only, a Stern-Brocot walk in integers.  None exists, or value, rel_tol not finite, value <= 0, rel_tol < 0 or
 * >= 1, a zero maximum: GR4PM_ERR_INVALID (num and den are then 0). */
gr4pm_status gr4pm_simplest_ratio(double value, double rel_tol, uint32_t max_num, uint32_t max_den, uint32_t* num,
                                  uint32_t* den);

/* ====================================================================================
 * RowResampler -- rows of channel items to any real rate with the residual carrier removed, every row with a
 * step and a frequency of its own (the project's own block).  It is what acts on a
 * LineSpectrum's per-row symbol rate and offset where they were measured: on the burst rows of
 * gr4pm_ddc_extract, without going back to the wideband recording.
 *
 * Handle: Q phases, a power of two 2 .. 256; P taps per phase, 1 <= P, Q P <= 4096; a real prototype
 * h[0 .. Q P - 1] at the virtual rate Q per input item, copied from HOST floats at create, h[Q P] = 0.  Two float
 * tables are made on the host:
 *     H[q][s]  = h[s Q + q]
 *     Dh[q][s] = fl32(h[s Q + q + 1] - h[s Q + q])       the difference in double from the float taps, rounded once
 * Call: R <= 64 rows x[r stride + i] of DEVICE complex64, row r with n_r = lengths[r] items, and R HOST records
 * {step, phase0, freq}, which travel to the kernel by value.  step and phase0 are positions in input items with 32
 * fractional bits, 2^26 <= step <= 2^38 (1/64 .. 64 input items per output item); freq is the SIGNED frequency
 * word, cycles per input item times 2^32 (the position has fractional bits, so w and w - 2^32 are not the same
 * frequency here).  Output item m of row r, with b = 32 - log2 Q:
 *     pos   = phase0 + m step                             exact in 64 bits
 *     i     = pos >> 32,  mu = pos & 0xffffffff,  q = mu >> b
 *     alpha = fl32(mu & (2^b - 1)) 2^-b                   the conversion rounds to nearest; alpha may round to 1
 *     c_s   = fmaf(alpha, Dh[q][s], H[q][s])
 *     acc   = sum_{s=0}^{P-1} c_s x_r[i - s]              one accumulator from +0, s ascending:
 *                                                         re = fmaf(c_s, x.re, re), im = fmaf(c_s, x.im, im)
 *     theta = (freq (pos >> 32) + ((int64(freq) int64(mu)) >> 32)) mod 2^32      the shift is arithmetic:
 *                                                         theta = floor(freq pos / 2^32) mod 2^32
 *     y_r[m] = exp(-2 pi j theta / 2^32) acc              the Ddc's rotator: double sincospi of -theta / 2^31, an
 *                                                         exact argument, rounded to float; four fmaf from zero
 * A sample with i - s < 0 or i - s >= n_r is the operand +0 and IS NEVER LOADED: a row may end at its buffer's last
 * byte and may hold anything behind n_r.  The mix comes AFTER the filter and the filter is not re-centred: the
 * block is for residual offsets well inside the prototype's passband.  A tone at the input appears
 * (Q P - 1) / (2 Q) input items late.
 * Output length: M_r is the number of m with pos >> 32 <= n_r + P - 2 (the filter runs out over the row's end):
 * 0 if n_r = 0 or phase0 is beyond that, and cut at n_cols_out.  out[r out_stride + m] = y_r[m] for m < M_r and +0
 * up to n_cols_out; out may be uninitialised.  M_r is computed on the host.
 * A ROW'S RESULT DEPENDS ON THAT ROW ALONE, BIT FOR BIT, not on the rows beside it or on R; and items m0 .. of a call
 * equal items 0 .. of a call with phase0 + m0 step: nothing depends on the tile an item falls in.
 * ================================================================================== */
typedef struct gr4pm_row_resampler gr4pm_row_resampler;
typedef struct {
    uint64_t step;              /* input items per output item, Q32.32: 2^26 .. 2^38 */
    uint64_t phase0;            /* position of output item 0, Q32.32: below 2^63 */
    int32_t freq;               /* cycles per input item times 2^32, signed */
} gr4pm_row_record;
typedef struct {
    uint32_t phases;            /* Q */
    uint32_t taps_per_phase;    /* P (0 with NULL taps: 12) */
    const float* taps;          /* host: Q P floats, copied at create (NULL: gr4pm_row_resampler_taps(Q, P, 1, 0.25, 0.75)) */
    void* stream;               /* hipStream_t (NULL: the default stream) */
} gr4pm_row_resampler_params;
/* The prototype, host only: the Kaiser design of gr4pm_ddc_taps at the virtual rate with DC gain Q.  The band edges
 * are in units of the lower of the input rate and the output rate at max_step (input items per output item, 1/64 ..
 * 64): they are divided by max(1, max_step), and the span is P = ceil(taps_per_phase max(1, max_step)) taps per
 * phase, so a decimating handle keeps the design's span in output items.  out: room for Q P floats.  A Q that is
 * no power of two in 2 .. 256, taps_per_phase == 0, Q P > 4096, a max_step out of range or not finite, or edges
 * without 0 <= passband < stopband and passband + stopband <= 1: GR4PM_ERR_INVALID. */
gr4pm_status gr4pm_row_resampler_taps(size_t phases, size_t taps_per_phase, double max_step, double passband,
                                      double stopband, float* out);
/* a bad Q, Q P > 4096 or a non-finite tap: GR4PM_ERR_INVALID, no handle */
gr4pm_status gr4pm_row_resampler_create(const gr4pm_row_resampler_params* params, gr4pm_row_resampler** out);
void gr4pm_row_resampler_destroy(gr4pm_row_resampler* h);
/* Host only, no handle: out_lengths[r] = M_r of a handle with taps_per_phase = P for the rows' lengths (HOST, NULL:
 * n_cols each) and records, cut at n_cols_out.  Refuses what gr4pm_row_resampler_process refuses of them. */
gr4pm_status gr4pm_row_resampler_output_lengths(size_t taps_per_phase, size_t n_cols, const uint64_t* lengths,
                                                const gr4pm_row_record* rows, size_t n_rows, size_t n_cols_out,
                                                uint64_t* out_lengths);
/* Host only: the output items of a tile of a call whose largest step is max_step, for P taps per phase; 0 for
 * arguments a call would refuse.  Nothing depends on it but the time a call takes. */
uint32_t gr4pm_row_resampler_tile_items(size_t taps_per_phase, uint64_t max_step);
/* x: DEVICE, R rows of n_cols items, `stride` items apart.  lengths: HOST, R items, copied by the call (NULL: every
 * row has n_cols items).  rows: HOST, R records, copied by the call.  out: DEVICE, R rows of n_cols_out items,
 * out_stride apart.  out_lengths: HOST, R items: M_r.  Enqueues on the handle's stream, does not wait and reads
 * nothing back.  Refused with gr4pm_last_error set and nothing enqueued -- GR4PM_ERR_INVALID: R > 64, a length above
 * n_cols, R > 1 with stride < n_cols or out_stride < n_cols_out, a step out of range, a NULL rows, out_lengths or
 * out, a NULL x when any length is not zero; GR4PM_ERR_OVERFLOW: n_r + P - 1 >= 2^32, phase0 >= 2^63,
 * n_cols_out > 2^31.  R = 0 or n_cols_out = 0: OK, nothing enqueued. */
gr4pm_status gr4pm_row_resampler_process(gr4pm_row_resampler* h, const gr4pm_c64* x, size_t stride, size_t n_cols,
                                         const uint64_t* lengths, const gr4pm_row_record* rows, size_t n_rows,
                                         gr4pm_c64* out, size_t out_stride, size_t n_cols_out, uint64_t* out_lengths);

/* ====================================================================================
 * StreamRowResampler (gr4pm_row_stream) -- the RowResampler as a stream block: every row's position, history and
 * phase are carried from call to call, and CUTTING THE ROWS INTO CALLS CHANGES NO BIT OF WHAT COMES OUT (the
 * project's own block).  It closes the chain MixedFftDdc -> rows at 4 samples per symbol ->
 * one receiver per row for recordings of any length and carriers of any symbol rate.
 *
 * Handle: the RowResampler's prototype and the two tables made from it: Q phases, P taps per phase, the same H and
 * Dh, the same refusals of the sizes, NULL taps the same default design.  R = 1 .. 64 rows, each with a record
 * {step, phase0, freq}, a gr4pm_row_record: the step's range is the one-shot's and phase0 < 2^63; and a start_index[r]
 * (uint64; a NULL array: 0 for every row): the absolute index of the first item the row will ever be given, as the
 * MixedFftDdc has a start_index.
 * A row is an unbounded sequence of items x_r[a], a an absolute index; every x_r[a] with a < start_index[r] is +0.
 * Output item m sits at pos_m = phase0 + m step, an unbounded integer with 32 fractional bits.  Its value is the
 * RowResampler's: the branch, alpha, c_s, the single accumulator with s ascending and the rotator are unchanged, with
 *     theta(pos) = Phi + floor(freq (pos - ref) / 2^32) mod 2^32
 * At create Phi = 0 and ref = 0, so theta is the one-shot's floor(freq pos / 2^32) mod 2^32.
 * Per-row state: A_r, the items taken so far (it starts at start_index[r]); the index of the next output item and
 * its position (at create the first m with floor(pos_m) >= start_index[r]); Phi, ref, and the row's last P - 1 items
 * on the device (+0 at create).
 * process: the next lengths[r] <= n_cols items of each row, the layout gr4pm_fft_ddc_mixed_process returns.  Row r
 *   makes every item not yet made with floor(pos) <= A_r + lengths[r] - 1, into out[r out_stride + 0 ..] with +0
 *   behind them up to n_cols_out (out may be uninitialised), and their count into out_lengths[r].  Rows are
 *   independent; any mix of lengths in one call, 0 and lengths below P - 1 included.
 * flush: the items with floor(pos) <= A_r + P - 2 (the filter runs out over +0 behind the last item, as the one-
 *   shot's M_r does), then every row is back in its created state with its current step and freq.
 * reset: the same without the output.
 * set_row(r, step, freq) takes effect at the next output item: with m* its index, its position p* does not move,
 *   pos_m = p* + (m - m*) step_new from then on, Phi <- theta_old(p*), ref <- p*, freq <- freq_new: the phase is
 *   continuous at item m*.
 * items_for: host only, changes no state: what the next process would report for these lengths.
 * state: the row's two counters, A_r and the index of the next output item (mod 2^64).
 * The host's exact arithmetic: the kernel works with 64-bit positions relative to a per-call base.  The host moves the
 * base, and ref with it, forward by whole items B and adds freq B mod 2^32 to Phi:
 *     floor(freq (pos - ref - B 2^32) / 2^32) = floor(freq (pos - ref) / 2^32) - freq B
 * so no theta changes, and no position wraps however long the stream is.
 * Refusals enqueue nothing and change no state.  GR4PM_ERR_INVALID: a row count outside 1 .. 64, a step out of range
 * (create, set_row), lengths[r] > n_cols, R > 1 with stride < n_cols or out_stride < n_cols_out, a NULL array that is
 * needed.  GR4PM_ERR_OVERFLOW: phase0 >= 2^63, lengths[r] + P - 1 >= 2^32, n_cols_out > 2^31, an n_cols_out below some
 * row's count of this call (a stream must not lose items, so the call is not cut).  Calls enqueue on the handle's
 * stream, do not wait and read nothing back.  create, items_for, set_row, state and reset are host only: the device
 * tables are made by the first process or flush, which is where a missing device is an error.
 * ================================================================================== */
typedef struct gr4pm_row_stream gr4pm_row_stream;
typedef struct {
    uint32_t phases;               /* Q */
    uint32_t taps_per_phase;       /* P (0 with NULL taps: 12) */
    const float* taps;             /* host: Q P floats, copied at create (NULL: gr4pm_row_resampler_taps(Q, P, 1, 0.25, 0.75)) */
    size_t n_rows;                 /* R: 1 .. 64 */
    const gr4pm_row_record* rows;  /* host: R records, copied at create */
    const uint64_t* start_index;   /* host: R absolute indices (NULL: 0 each) */
    void* stream;                  /* hipStream_t (NULL: the default stream) */
} gr4pm_row_stream_params;
gr4pm_status gr4pm_row_stream_create(const gr4pm_row_stream_params* params, gr4pm_row_stream** out);
void gr4pm_row_stream_destroy(gr4pm_row_stream* h);
gr4pm_status gr4pm_row_stream_reset(gr4pm_row_stream* h);
/* lengths, out_lengths: HOST, R items each */
gr4pm_status gr4pm_row_stream_items_for(const gr4pm_row_stream* h, const uint64_t* lengths, uint64_t* out_lengths);
/* x: DEVICE, R rows of n_cols items, `stride` items apart (may be NULL when every length is 0).  lengths: HOST, R items
 * (NULL: n_cols each).  out: DEVICE, R rows of n_cols_out items, out_stride apart (may be NULL when n_cols_out is 0).
 * out_lengths: HOST, R items. */
gr4pm_status gr4pm_row_stream_process(gr4pm_row_stream* h, const gr4pm_c64* x, size_t stride, size_t n_cols,
                                      const uint64_t* lengths, gr4pm_c64* out, size_t out_stride, size_t n_cols_out,
                                      uint64_t* out_lengths);
gr4pm_status gr4pm_row_stream_flush(gr4pm_row_stream* h, gr4pm_c64* out, size_t out_stride, size_t n_cols_out,
                                    uint64_t* out_lengths);
gr4pm_status gr4pm_row_stream_set_row(gr4pm_row_stream* h, size_t row, uint64_t step, int32_t freq);
gr4pm_status gr4pm_row_stream_state(const gr4pm_row_stream* h, size_t row, uint64_t* items_in, uint64_t* items_out);

/* ====================================================================================
 * RowBurstGate (gr4pm_row_gate) -- a power squelch on rows that carries its state from call to call: fed with the
 * ragged rows of gr4pm_fft_ddc_mixed_process call after call, it delivers every burst of every row once, as a
 * zero-padded row of the [bursts, n_cols] layout that the LineSpectrum, the RowResampler and the receivers take.
 * CUTTING THE ROWS INTO CALLS CHANGES NO BYTE OF A ROW'S RECORDS AND BURST ROWS (the project's own block; DESIGN.md
 * section 30).
 *
 * Handle: R = 1 .. 64 rows of complex64 items and a block length B, a power of two from 16 to 1024 (0: 64).  Each
 * row counts its items from 0 at create, reset and flush, as uint64; block b of a row is its items [b B, (b + 1) B).
 * Block power, bit for bit: per item p = fl32(fl32(re re) + fl32(im im)), no contraction.  The block sum s_b is
 * float32 over the B values in this order, fixed per B: with W = min(B, 64), t[l] (l = 0 .. W - 1) takes p of the
 * block's item l and then adds those of items l + W, l + 2 W, ... in ascending order, one float32 addition each;
 * then log2(W) folds with offset = W / 2, W / 4, .. 1: t[l] <- fl32(t[l] + t[l + offset]) for l < offset; s_b = t[0].
 * It does not depend on how the row is cut into calls.
 * Per-row state machine over s_b in block order; comparisons are float32 against the row's open_sum and close_sum,
 * 0 < close_sum <= open_sum (a NaN sum compares false: inactive).
 *   idle: a block with s_b >= open_sum opens a burst: first_active = last_active = b, start = max(0, b - pre_blocks).
 *   open: a block with s_b >= close_sum is active: last_active = b.  The (hold_blocks + 1)-th inactive block in a row
 *     closes the burst: with last_active - first_active + 1 < min_blocks it is dropped and counted, else the span of
 *     blocks [start, last_active + post_blocks] is emitted.  post_blocks <= hold_blocks + 1, so the post margin has
 *     arrived at the closing block, and a burst is emitted in the call that holds its closing block.
 *   forced split: a block c behind which the burst is still open and with c - start + 1 == max_blocks ends it: the
 *     span [start, c] is emitted with GR4PM_ROW_GATE_TRUNCATED whatever its active extent, the row goes idle and
 *     the next block is judged from idle; its pre margin may reach back into the emitted span (a copy, no error).
 *     No span exceeds max_blocks blocks.
 *   set_thresholds(row, open_sum, close_sum) holds from the next block decided.
 * create refuses (GR4PM_ERR_INVALID) R outside 1 .. 64, a B that is no power of two in 16 .. 1024, min_blocks = 0,
 * post_blocks > hold_blocks + 1, pre_blocks + min_blocks + post_blocks > max_blocks, max_blocks B > n_cols,
 * n_cols > 2^30, and sums other than 0 < close_sum <= open_sum (both 0: the gate stays shut until set_thresholds).
 * process appends lengths[r] <= stride items to row r.  Items of an incomplete trailing block are kept and have no
 *   power yet.  Per emitted burst, in the order (row, time) within a call, out[i out_stride + 0 .. n_items) holds the
 *   span's items and +0 fills the rest up to n_cols (out may be uninitialised; rows at and behind *n_bursts are not
 *   touched), and records[i] goes with it: row, first_item (of the span), n_items, first_active_item, active_items
 *   ((last_active - first_active + 1) B), flags, peak (the largest s_b of the active extent) and power (the sum of the
 *   active blocks' s_b in block order, in double on the host, divided by active_items).
 *   Capacity: a call that emits more than `cap` bursts returns GR4PM_ERR_OVERFLOW with the count in *n_bursts and
 *   changes nothing: the plan is made before anything is committed, so the same call with that cap succeeds.  Every
 *   other refusal leaves the state untouched too: a NULL array that is needed (GR4PM_ERR_INVALID), lengths[r] >
 *   stride (GR4PM_ERR_INVALID), lengths[r] >= 2^32 - max_blocks B (GR4PM_ERR_OVERFLOW), cap > 1 with out_stride <
 *   n_cols (GR4PM_ERR_INVALID).
 * flush: a trailing incomplete block is completed with +0 for its power only and decided; then the row counts as
 *   followed by inactive blocks without end: an open burst closes at once (dropped below min_blocks), with
 *   GR4PM_ROW_GATE_AT_END and its post margin, n_items and active_items clipped to the items that exist.  What closes
 *   is emitted as process emits; then every row is in its created state, its thresholds and burst counters kept.
 * reset: the created state (counters at 0) without emitting; the thresholds stay.
 * state: items taken, blocks decided, open or idle, bursts emitted, dropped and truncated.
 * block_power: a one-shot entry that changes no state: the floor(lengths[r] / B) block sums of rows that begin at
 *   item 0, into out[r out_stride + b]: the same kernel body, the same bits.  Enqueues and does not wait.
 * Per row, the sequence of records and the bytes of the burst rows do not depend on the cutting into calls; only the
 * interleaving of different rows' bursts across calls does.  A row retains at most (max_blocks + 1) B - 1 items on
 * the device.  process and flush enqueue on the handle's stream, copy the call's block sums to the host and wait for
 * them once, in front of the plan; the copies into `out` are enqueued behind it and not waited for, so x lives until
 * the stream has run them.  create, set_thresholds, state, sizes and reset are host only: the device side is made by
 * the first process, flush or block_power, which is where a missing device is an error.
 * ================================================================================== */
#define GR4PM_ROW_GATE_TRUNCATED 1u
#define GR4PM_ROW_GATE_AT_END 2u
typedef struct gr4pm_row_gate gr4pm_row_gate;
typedef struct {
    size_t n_rows;        /* R: 1 .. 64 */
    size_t n_cols;        /* columns of a burst row */
    uint32_t block;       /* B (0: 64) */
    uint32_t hold_blocks;
    uint32_t min_blocks;
    uint32_t pre_blocks;
    uint32_t post_blocks;
    uint32_t max_blocks;  /* 0: n_cols / B */
    float open_sum;       /* every row's at create (both 0: +inf, shut) */
    float close_sum;
    void* stream;         /* hipStream_t (NULL: the default stream) */
} gr4pm_row_gate_params;
typedef struct {
    uint64_t first_item;        /* of the span, counted in the row */
    uint64_t first_active_item;
    double power;               /* per item of the active extent */
    uint32_t row;
    uint32_t n_items;
    uint32_t active_items;
    uint32_t flags;             /* GR4PM_ROW_GATE_* */
    float peak;
    uint32_t reserved;
} gr4pm_row_gate_record;
typedef struct {
    uint64_t items, blocks, emitted, dropped, truncated;
    uint32_t open;
    uint32_t reserved;
} gr4pm_row_gate_state_t;
gr4pm_status gr4pm_row_gate_create(const gr4pm_row_gate_params* params, gr4pm_row_gate** out);
void gr4pm_row_gate_destroy(gr4pm_row_gate* h);
gr4pm_status gr4pm_row_gate_reset(gr4pm_row_gate* h);
gr4pm_status gr4pm_row_gate_set_thresholds(gr4pm_row_gate* h, size_t row, float open_sum, float close_sum);
gr4pm_status gr4pm_row_gate_state(const gr4pm_row_gate* h, size_t row, gr4pm_row_gate_state_t* out);
gr4pm_status gr4pm_row_gate_sizes(const gr4pm_row_gate* h, uint32_t* block, uint32_t* max_blocks, size_t* n_cols);
/* x: DEVICE, R rows `stride` items apart (may be NULL when every length is 0).  lengths: HOST, R items.  out: DEVICE,
 * cap rows of n_cols items, out_stride apart.  records: HOST, cap records.  n_bursts: HOST. */
gr4pm_status gr4pm_row_gate_process(gr4pm_row_gate* h, const gr4pm_c64* x, size_t stride, const uint64_t* lengths,
                                    gr4pm_c64* out, size_t out_stride, size_t cap, gr4pm_row_gate_record* records,
                                    size_t* n_bursts);
gr4pm_status gr4pm_row_gate_flush(gr4pm_row_gate* h, gr4pm_c64* out, size_t out_stride, size_t cap,
                                  gr4pm_row_gate_record* records, size_t* n_bursts);
/* out: DEVICE float, R rows out_stride apart */
gr4pm_status gr4pm_row_gate_block_power(gr4pm_row_gate* h, const gr4pm_c64* x, size_t stride, const uint64_t* lengths,
                                        float* out, size_t out_stride);

/* ---- FftDdc: K off-grid channels from one shared transform (the project's own block) ----------
 * The Ddc's drop-in for power-of-two decimations and many channels: a fast-convolution (overlap-save) filter bank.
 * N = 2048, K channels (1 .. 64), D a power of two in 4 .. 64, B = N / D, a real finite prototype h[0 .. L - 1], an
 * overlap V with D | V and L - 1 <= V <= N - 64 (overlap < 0: the smallest multiple of 256 that is >= L - 1),
 * hop = N - V, images = R, a power of two with 1 <= R <= D.  x[i] = 0 before the handle's first sample, whose absolute
 * index is start_index.
 *     w_k = llrint(f_k 2^32) mod 2^32,   c_k = floor(w_k N / 2^32 + 1 / 2) mod N   (the nearest bin, in integers)
 *     segment s: the N items from a_s = s hop - V + D - 1 on (relative to the first sample),  X_s = FFT_N(x_s)
 *         (forward, unnormalised, no window)
 *     G_k[u] = (1 / N) sum_t h[t] exp(-2 pi j ((c_k + u) / N - w_k / 2^32) t),   u in [-R B / 2, R B / 2)
 *         (host, double, each component rounded to float once)
 *     Z[u] = X_s[(c_k + u) mod N] G_k[u],   Y[v] = sum_{u = v mod B} Z[u]  (R terms, ascending u)
 *     y'[n'] = sum_v Y[v] exp(+2 pi j v n' / B),   n' = V / D .. B - 1 are kept: hop / D frames a segment
 *     p = n' D,   i = start_index + a_s + p,   phi = (w_k i - c_k 2^21 p) mod 2^32   (wrapping integers)
 *     out_k[s hop / D + n' - V / D] = exp(-2 pi j phi / 2^32) y'[n']   (the Ddc's rotator: double sincospi of the
 *         exact argument rounded to float, then four fmaf from zero)
 * Frame n of row k lies at i = start_index + n D + D - 1, the Ddc's own frame grid.  With R = D the definition is the
 * Ddc's y_k[n] in exact arithmetic; with R < D it differs by the prototype's response outside +-R / (2 D) cycles per
 * sample: |y - y_Ddc| <= ||x_s||_2 ||H_k outside the slice||_2 / sqrt(N).  R = 1 cuts inside the default design's
 * transition band; it is accepted.  A call delivers whole segments, hop / D frames each; the handle carries V samples
 * plus the incomplete hop, and any cutting of the stream into calls gives the same bits. */
typedef struct gr4pm_fft_ddc gr4pm_fft_ddc;
typedef struct {
    size_t n_channels;          /* K: 1 .. 64 */
    size_t decimation;          /* D: a power of two, 4 .. 64 */
    const double* frequencies;  /* HOST, K items, cycles per input sample, finite */
    const float* taps;          /* HOST, n_taps items, finite; NULL: gr4pm_fft_ddc_taps(D, taps_per_phase) */
    size_t n_taps;              /* L */
    size_t taps_per_phase;      /* of the design when taps is NULL */
    int64_t overlap;            /* V; negative: the default */
    size_t images;              /* R */
    uint64_t start_index;
    void* stream;               /* hipStream_t */
} gr4pm_fft_ddc_params;
/* Host only: the Ddc's design (gr4pm_ddc_taps with the band edges 0.25 and 0.75 of the output rate) of
 * taps_per_phase * decimation floats for a decimation the FftDdc takes. */
gr4pm_status gr4pm_fft_ddc_taps(size_t decimation, size_t taps_per_phase, float* out);
/* Refused with GR4PM_ERR_INVALID and no handle: K out of range, a NULL or non-finite frequency, D or R no power of two
 * or out of range, a non-finite tap, n_taps out of range, V no multiple of D, below L - 1 or above N - 64. */
gr4pm_status gr4pm_fft_ddc_create(const gr4pm_fft_ddc_params* params, gr4pm_fft_ddc** out);
void gr4pm_fft_ddc_destroy(gr4pm_fft_ddc* h);
/* back to start_index: zero prehistory, nothing carried */
gr4pm_status gr4pm_fft_ddc_reset(gr4pm_fft_ddc* h);
/* frames per row the next call of n_in samples delivers */
gr4pm_status gr4pm_fft_ddc_frames_for(const gr4pm_fft_ddc* h, size_t n_in, size_t* n_frames);
/* out: HOST, K items: w_k / 2^32 folded to [-0.5, 0.5) */
gr4pm_status gr4pm_fft_ddc_frequencies(const gr4pm_fft_ddc* h, double* out);
gr4pm_status gr4pm_fft_ddc_sizes(const gr4pm_fft_ddc* h, size_t* overlap, size_t* hop);
/* in: DEVICE, n_in samples.  out: DEVICE, K rows out_stride items apart with room for out_cap_frames each.  Enqueues on
 * the handle's stream and does not wait.  Refused with gr4pm_last_error set, *n_frames = 0 and nothing enqueued: a NULL
 * in with n_in > 0, a NULL out or out_stride below the frames with K > 1 when the call delivers frames
 * (GR4PM_ERR_INVALID); n_in > 2^40 or fewer than the frames of room (GR4PM_ERR_OVERFLOW).  The handle stays usable. */
gr4pm_status gr4pm_fft_ddc_process(gr4pm_fft_ddc* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_stride,
                                   size_t out_cap_frames, size_t* n_frames);
/* The same for integer IQ (GR4PM_IQ_SC16 / SC8 / CU8; scale 0: the format's default): gr4pm_fft_ddc_process on
 * gr4pm_iq_unpack(in) bit for bit; calls of any format mix on one handle. */
gr4pm_status gr4pm_fft_ddc_process_iq(gr4pm_fft_ddc* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                      size_t out_stride, size_t out_cap_frames, size_t* n_frames);

/* ---- MixedFftDdc: a decimation per channel from one shared transform (the project's own block) --
 * The FftDdc with its restriction to one decimation lifted: carriers of different symbol rates in one pass over the
 * stream.  N = 2048, K channels (1 .. 64); channel k has a frequency f_k, D_k a power of two in 4 .. 64, B_k = N / D_k, a
 * real finite prototype h_k[0 .. L_k - 1] and R_k images, a power of two with 1 <= R_k <= D_k.  Dmax = max D_k.  One
 * overlap V for the handle with Dmax | V, V <= N - 64 and V - (Dmax - D_k) >= L_k - 1 for every k (overlap < 0: the
 * smallest multiple of 256 that is >= max_k (Dmax - D_k + L_k - 1)), hop = N - V.  All channels share one segment
 * grid, anchored on Dmax:
 *     segment s: the N items from a_s = s hop - V + Dmax - 1 on (x = 0 before start_index),  X_s = FFT_N(x_s)
 *     w_k, c_k, G_k[u], Z[u], Y[v], y'[n']: the FftDdc's with h_k, B_k, R_k in the place of h, B, R
 *     first_k = (V - Dmax) / D_k + 1,   n' = first_k .. first_k + hop / D_k - 1 are kept
 *     p = n' D_k,   i = start_index + a_s + p,   phi = (w_k i - c_k 2^21 p) mod 2^32
 *     out_k[s hop / D_k + n' - first_k] = exp(-2 pi j phi / 2^32) y'[n']
 * Frame n of row k lies at i = start_index + n D_k + D_k - 1, the Ddc's frame grid at D_k, so row k is
 * Ddc([f_k], D_k, taps = h_k) from frame 0 on, up to the truncation to R_k images (the FftDdc's bound).  With all D_k
 * equal the block is the FftDdc, bit for bit.  A call delivers whole segments, hop / D_k frames of row k each; the handle
 * carries V samples plus the incomplete hop, and any cutting of the stream into calls gives the same bits. */
typedef struct gr4pm_fft_ddc_mixed gr4pm_fft_ddc_mixed;
typedef struct {
    size_t n_channels;          /* K: 1 .. 64 */
    const size_t* decimations;  /* HOST, K items: D_k, powers of two, 4 .. 64 */
    const double* frequencies;  /* HOST, K items, cycles per input sample, finite */
    const float* taps;          /* HOST, the K prototypes behind one another, finite; NULL together with n_taps:
                                   gr4pm_fft_ddc_taps(D_k, taps_per_phase) per channel */
    const size_t* n_taps;       /* HOST, K items: L_k */
    size_t taps_per_phase;      /* of the design when taps is NULL */
    const size_t* images;       /* HOST, K items: R_k; NULL: 2 each */
    int64_t overlap;            /* V; negative: the default */
    uint64_t start_index;
    void* stream;               /* hipStream_t */
} gr4pm_fft_ddc_mixed_params;
/* Refused with GR4PM_ERR_INVALID and no handle: K out of range, a NULL or non-finite frequency, no decimations, taps
 * without n_taps or the reverse, a D_k or R_k no power of two or out of range, a non-finite tap, an L_k out of range, V
 * no multiple of Dmax, above N - 64, or below Dmax - D_k + L_k - 1 for a channel k. */
gr4pm_status gr4pm_fft_ddc_mixed_create(const gr4pm_fft_ddc_mixed_params* params, gr4pm_fft_ddc_mixed** out);
void gr4pm_fft_ddc_mixed_destroy(gr4pm_fft_ddc_mixed* h);
/* back to start_index: zero prehistory, nothing carried */
gr4pm_status gr4pm_fft_ddc_mixed_reset(gr4pm_fft_ddc_mixed* h);
/* n_frames: HOST, K items: the frames of each row the next call of n_in samples delivers */
gr4pm_status gr4pm_fft_ddc_mixed_frames_for(const gr4pm_fft_ddc_mixed* h, size_t n_in, size_t* n_frames);
/* out: HOST, K items: w_k / 2^32 folded to [-0.5, 0.5) */
gr4pm_status gr4pm_fft_ddc_mixed_frequencies(const gr4pm_fft_ddc_mixed* h, double* out);
gr4pm_status gr4pm_fft_ddc_mixed_sizes(const gr4pm_fft_ddc_mixed* h, size_t* overlap, size_t* hop);
/* in: DEVICE, n_in samples.  out: DEVICE, K rows out_stride items apart with room for out_cap_frames each.  n_frames:
 * HOST, K items.  Row k receives n_frames[k] frames and behind them +0 up to max_k n_frames[k], written by the same
 * kernel: rows go to a receiver zero-padded.  Enqueues on the handle's stream and does not wait.  Refused with
 * gr4pm_last_error set, every n_frames[k] = 0 and nothing enqueued: a NULL in with n_in > 0, a NULL out or out_stride
 * below the longest row with K > 1 when the call delivers frames (GR4PM_ERR_INVALID); n_in > 2^40 or less room than the
 * longest row (GR4PM_ERR_OVERFLOW).  The handle stays usable. */
gr4pm_status gr4pm_fft_ddc_mixed_process(gr4pm_fft_ddc_mixed* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_stride,
                                         size_t out_cap_frames, size_t* n_frames);
/* The same for integer IQ (GR4PM_IQ_SC16 / SC8 / CU8; scale 0: the format's default): gr4pm_fft_ddc_mixed_process on
 * gr4pm_iq_unpack(in) bit for bit; calls of any format mix on one handle. */
gr4pm_status gr4pm_fft_ddc_mixed_process_iq(gr4pm_fft_ddc_mixed* h, const void* in, int format, float scale, size_t n_in,
                                            gr4pm_c64* out, size_t out_stride, size_t out_cap_frames, size_t* n_frames);

/* ---- FftDuc: K carriers onto one stream from one shared transform (the project's own block) ----
 * The Duc's drop-in for power-of-two interpolations and many channels, the mirror of the FftDdc: a fast-convolution
 * (overlap-save) synthesis bank.  N = 2048, K channels (1 .. 64), I a power of two in 4 .. 64, B = N / I, a real finite
 * prototype h[0 .. L - 1] (NULL: gr4pm_duc_taps(I, taps_per_phase, 0.25, 0.75), DC gain I), real finite gains a_k
 * (NULL: all 1), an overlap V with I | V and L - 1 <= V <= N - 64 (overlap < 0: the smallest multiple of 256 that is
 * >= L - 1), hop = N - V, hopI = hop / I, images = R, a power of two with 1 <= R <= I.  start_index: the absolute index
 * of the first output sample.  v_k[m] = 0 for m < 0.
 *     w_k = llrint(f_k 2^32) mod 2^32,   c_k = floor(w_k N / 2^32 + 1 / 2) mod N   (the nearest bin, in integers)
 *     z_k[m] = q_k[m] v_k[m],   q_k[m] = exp(+2 pi j ((w_k (start_index + m I)) mod 2^32) / 2^32)
 *         (the Duc's rotator: double sincospi of the exact argument rounded to float, then four fmaf from zero)
 *     segment s: the output samples j = a_s .. a_s + N - 1, a_s = s hop - V; the input items m = a_s / I + n', n' < B
 *     Z_k[v] = sum_n' z_k[a_s / I + n'] exp(-2 pi j v n' / B),   v in [0, B)   (forward, unnormalised)
 *     G_k[u] = (a_k / N) sum_t h[t] exp(-2 pi j ((c_k + u) / N - w_k / 2^32) t),   u in [-R B / 2, R B / 2)
 *         (host, double, each component rounded to float once)
 *     S_s[b] = sum_k G_k[u] Z_k[b mod B] over the channels whose slice holds b = (c_k + u) mod N
 *         (one accumulator per bin, from zero, k ascending)
 *     x_s[p] = sum_b S_s[b] exp(+2 pi j b p / N);   p = V .. N - 1 are kept:   out[s hop + p - V] = x_s[p]
 * With R = I the definition is the Duc's x[start_index + j] in exact arithmetic; with R < I it differs by the
 * prototype's response outside +-R / (2 I) cycles per sample: |out - x_Duc| <= sum_k ||v_k over the segment||_2
 * ||H_k outside the slice||_2 / sqrt(N), H_k = N G_k.  Segment s is complete after (s + 1) hopI items per row; a call of
 * n_in items per row delivers whole segments, (floor((taken + n_in) / hopI) - floor(taken / hopI)) hop samples; the
 * handle carries V / I + (taken mod hopI) < B items per row, and any cutting of the rows into calls gives the same
 * bits. */
typedef struct gr4pm_fft_duc gr4pm_fft_duc;
typedef struct {
    size_t n_channels;          /* K: 1 .. 64 */
    size_t interpolation;       /* I: a power of two, 4 .. 64 */
    const double* frequencies;  /* HOST, K items, cycles per output sample, finite */
    const double* gains;        /* HOST, K items, finite; NULL: all 1 */
    const float* taps;          /* HOST, n_taps items, finite; NULL: gr4pm_fft_duc_taps(I, taps_per_phase) */
    size_t n_taps;              /* L */
    size_t taps_per_phase;      /* of the design when taps is NULL */
    int64_t overlap;            /* V; negative: the default */
    size_t images;              /* R */
    uint64_t start_index;
    void* stream;               /* hipStream_t */
} gr4pm_fft_duc_params;
/* Host only: the Duc's design (gr4pm_duc_taps with the band edges 0.25 and 0.75 of the input rate) of
 * taps_per_phase * interpolation floats for an interpolation the FftDuc takes. */
gr4pm_status gr4pm_fft_duc_taps(size_t interpolation, size_t taps_per_phase, float* out);
/* Refused with GR4PM_ERR_INVALID and no handle: K out of range, a NULL or non-finite frequency, a non-finite gain, I or
 * R no power of two or out of range, a non-finite tap, n_taps out of range, V no multiple of I, below L - 1 or above
 * N - 64. */
gr4pm_status gr4pm_fft_duc_create(const gr4pm_fft_duc_params* params, gr4pm_fft_duc** out);
void gr4pm_fft_duc_destroy(gr4pm_fft_duc* h);
/* back to start_index: zero prehistory, nothing carried */
gr4pm_status gr4pm_fft_duc_reset(gr4pm_fft_duc* h);
/* samples the next call of n_in items per row delivers */
gr4pm_status gr4pm_fft_duc_output_items(const gr4pm_fft_duc* h, size_t n_in, size_t* n_out);
/* out: HOST, K items: w_k / 2^32 folded to [-0.5, 0.5) */
gr4pm_status gr4pm_fft_duc_frequencies(const gr4pm_fft_duc* h, double* out);
gr4pm_status gr4pm_fft_duc_sizes(const gr4pm_fft_duc* h, size_t* overlap, size_t* hop);
/* items per row taken but not yet in a delivered segment: taken mod hopI */
gr4pm_status gr4pm_fft_duc_pending(const gr4pm_fft_duc* h, size_t* items);
/* in: DEVICE, K rows in_stride items apart, n_in items each.  out: DEVICE, room for out_cap samples.  Enqueues on the
 * handle's stream, reads nothing back and does not wait.  Refused with gr4pm_last_error set, *n_out = 0 and nothing
 * enqueued: a NULL in with n_in > 0, a NULL out when the call delivers samples, in_stride < n_in with K > 1
 * (GR4PM_ERR_INVALID); n_in > 2^40 or fewer than the samples of room (GR4PM_ERR_OVERFLOW).  The handle stays usable. */
gr4pm_status gr4pm_fft_duc_process(gr4pm_fft_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, gr4pm_c64* out,
                                   size_t out_cap, size_t* n_out);
/* The same call with the samples written as integer IQ, with gr4pm_duc_process_iq's contract:
 * out in items of `format`, out_cap in items, gain 0 the format's default, clipped NULL or a DEVICE counter the call
 * adds to; the bytes and the count are gr4pm_iq_pack's of what gr4pm_fft_duc_process would have written.  An unknown
 * format (GR4PM_ERR_INVALID) and whatever gr4pm_fft_duc_process refuses are refused before anything is enqueued. */
gr4pm_status gr4pm_fft_duc_process_iq(gr4pm_fft_duc* h, const gr4pm_c64* in, size_t in_stride, size_t n_in, void* out, int format,
                                      float gain, size_t out_cap, size_t* n_out, unsigned long long* clipped);

/* ---- MixedFftDuc: an interpolation per row into one shared transform (the project's own block) --
 * The FftDuc with its restriction to one interpolation lifted: carriers of different symbol rates onto one stream in one
 * pass.  N = 2048, K rows (1 .. 64); row k has a frequency f_k, I_k a power of two in 4 .. 64, B_k = N / I_k, a real finite
 * gain a_k, a real finite prototype h_k[0 .. L_k - 1] and R_k images, a power of two with 1 <= R_k <= I_k.  Imax = max
 * I_k.  One overlap V for the handle with Imax | V, V <= N - 64 and V >= L_k - 1 for every k (overlap < 0: the smallest
 * multiple of 256 that is >= max_k (L_k - 1)), hop = N - V.  Row k's item m sits at output sample m I_k; all rows start
 * at output sample 0, and v_k[m] = 0 for m < 0.
 *     w_k, c_k, G_k[u]: the FftDuc's with h_k, a_k, B_k, R_k in the place of h, a_k, B, R
 *     z_k[m] = exp(+2 pi j ((w_k (start_index + m I_k)) mod 2^32) / 2^32) v_k[m]
 *     segment s: the output samples a_s .. a_s + N - 1, a_s = s hop - V; row k's items m = a_s / I_k + n', n' < B_k
 *     Z_k[v] = the B_k-point forward transform of those items
 *     S_s[b] = sum_k G_k[u] Z_k[b mod B_k],  b = (c_k + u) mod N   (one accumulator per bin, from zero, k ascending)
 *     x_s = the inverse N-point transform of S_s;  p = V .. N - 1 are kept:  out[s hop + p - V] = x_s[p]
 * With R_k = I_k the output is sum_k Duc([f_k], I_k, taps = h_k, gains = [a_k])(v_k) in exact arithmetic; with all I_k
 * equal the block is the FftDuc, bit for bit.  The handle counts in slots of Imax output samples: a call of u slots takes
 * u Imax / I_k items of row k and delivers the whole segments they complete; it carries (V + pending Imax) / I_k < B_k
 * items of row k, and any cutting into calls gives the same bits. */
typedef struct gr4pm_fft_duc_mixed gr4pm_fft_duc_mixed;
typedef struct {
    size_t n_channels;            /* K: 1 .. 64 */
    const size_t* interpolations; /* HOST, K items: I_k, powers of two, 4 .. 64 */
    const double* frequencies;    /* HOST, K items, cycles per output sample, finite */
    const double* gains;          /* HOST, K items, finite; NULL: all 1 */
    const float* taps;            /* HOST, the K prototypes behind one another, finite; NULL together with n_taps:
                                     gr4pm_fft_duc_taps(I_k, taps_per_phase) per row */
    const size_t* n_taps;         /* HOST, K items: L_k */
    size_t taps_per_phase;        /* of the design when taps is NULL */
    const size_t* images;         /* HOST, K items: R_k; NULL: 2 each */
    int64_t overlap;              /* V; negative: the default */
    uint64_t start_index;
    void* stream;                 /* hipStream_t */
} gr4pm_fft_duc_mixed_params;
/* Refused with GR4PM_ERR_INVALID and no handle: K out of range, a NULL or non-finite frequency, no interpolations, a
 * non-finite gain, taps without n_taps or the reverse, an I_k or R_k no power of two or out of range, a non-finite tap, an
 * L_k out of range, V no multiple of Imax, above N - 64, or below L_k - 1 for a row k. */
gr4pm_status gr4pm_fft_duc_mixed_create(const gr4pm_fft_duc_mixed_params* params, gr4pm_fft_duc_mixed** out);
void gr4pm_fft_duc_mixed_destroy(gr4pm_fft_duc_mixed* h);
/* back to start_index: zero prehistory, nothing carried */
gr4pm_status gr4pm_fft_duc_mixed_reset(gr4pm_fft_duc_mixed* h);
/* items: HOST, K items: the items of each row a call of `slots` slots takes, slots Imax / I_k */
gr4pm_status gr4pm_fft_duc_mixed_items_for(const gr4pm_fft_duc_mixed* h, size_t slots, size_t* items);
/* samples the next call of `slots` slots delivers */
gr4pm_status gr4pm_fft_duc_mixed_output_items(const gr4pm_fft_duc_mixed* h, size_t slots, size_t* n_out);
/* out: HOST, K items: w_k / 2^32 folded to [-0.5, 0.5) */
gr4pm_status gr4pm_fft_duc_mixed_frequencies(const gr4pm_fft_duc_mixed* h, double* out);
gr4pm_status gr4pm_fft_duc_mixed_sizes(const gr4pm_fft_duc_mixed* h, size_t* overlap, size_t* hop);
/* slots taken but not yet in a delivered segment: taken mod (hop / Imax) */
gr4pm_status gr4pm_fft_duc_mixed_pending(const gr4pm_fft_duc_mixed* h, size_t* slots);
/* in: DEVICE, K rows in_stride items apart, slots Imax / I_k items in row k.  out: DEVICE, room for out_cap samples.
 * Enqueues on the handle's stream, reads nothing back and does not wait.  Refused with gr4pm_last_error set, *n_out = 0
 * and nothing enqueued: a NULL in with slots > 0, a NULL out when the call delivers samples, in_stride below the longest
 * row's items with K > 1 (GR4PM_ERR_INVALID); more than 2^40 items in the longest row or fewer than the samples of room
 * (GR4PM_ERR_OVERFLOW).  The handle stays usable. */
gr4pm_status gr4pm_fft_duc_mixed_process(gr4pm_fft_duc_mixed* h, const gr4pm_c64* in, size_t in_stride, size_t slots, gr4pm_c64* out,
                                         size_t out_cap, size_t* n_out);
/* The same call with the samples written as integer IQ: gr4pm_fft_duc_process_iq's contract on this handle */
gr4pm_status gr4pm_fft_duc_mixed_process_iq(gr4pm_fft_duc_mixed* h, const gr4pm_c64* in, size_t in_stride, size_t slots, void* out,
                                            int format, float gain, size_t out_cap, size_t* n_out, unsigned long long* clipped);

/* ---- FftFilter: any complex FIR on one wideband stream by fast convolution (the project's own block; DESIGN.md section
 * 32) ----
 * The same stream back with something removed: a CW interferer inside a channel, the DC spike of a recording, a strong
 * neighbour.  N = 2048, complex finite taps h[0 .. L - 1] with 1 <= L <= N - 63, an overlap V with L - 1 <= V <= N - 64 (any
 * integer; overlap 0: L - 1 rounded up to a multiple of 256, at most N - 64), hop = N - V.  x[i] = 0 for i < 0.
 *     segment s: the N items from s hop - V;   X_s = FFT_N(x_s)
 *     G[k] = (1 / N) sum_t h[t] exp(-2 pi j k t / N)   (host, double, each component rounded to float once)
 *     y_s = N IFFT_N(X_s G);   p = V .. N - 1 are kept:   out[s hop + p - V] = y_s[p]
 * So out[n] = sum_t h[t] x[n - t] in exact arithmetic: the causal filter, output sample n beside input sample n.  Segment s
 * is complete after (s + 1) hop samples; a call of n_in samples delivers whole segments, ((pending + n_in) / hop) hop
 * samples, the handle carries V + pending < N items, and any cutting of the stream into calls gives the same bits. */
typedef struct gr4pm_fft_filter gr4pm_fft_filter;
typedef struct {
    const gr4pm_c64* taps; /* HOST, n_taps items, finite */
    size_t n_taps;         /* L: 1 .. 1985 */
    size_t overlap;        /* V; 0: the default */
    void* stream;          /* hipStream_t */
} gr4pm_fft_filter_params;
/* Refused with GR4PM_ERR_INVALID and no handle: no taps, more than N - 63, a non-finite tap, V below L - 1 or above N - 64. */
gr4pm_status gr4pm_fft_filter_create(const gr4pm_fft_filter_params* params, gr4pm_fft_filter** out);
void gr4pm_fft_filter_destroy(gr4pm_fft_filter* h);
/* the fresh stream: zero prehistory, nothing pending */
gr4pm_status gr4pm_fft_filter_reset(gr4pm_fft_filter* h);
/* Other taps from the next segment delivered on; V, hop and the carried samples stay.  Refused with GR4PM_ERR_INVALID and the
 * handle unchanged: no taps, a non-finite tap, n_taps - 1 > V.  Waits for the handle's stream. */
gr4pm_status gr4pm_fft_filter_set_taps(gr4pm_fft_filter* h, const gr4pm_c64* taps, size_t n_taps);
gr4pm_status gr4pm_fft_filter_sizes(const gr4pm_fft_filter* h, size_t* overlap, size_t* hop, size_t* n_taps);
/* samples taken whose outputs are still owed: taken mod hop */
gr4pm_status gr4pm_fft_filter_pending(const gr4pm_fft_filter* h, size_t* samples);
/* samples the next call of n_in samples delivers */
gr4pm_status gr4pm_fft_filter_output_items(const gr4pm_fft_filter* h, size_t n_in, size_t* n_out);
/* in: DEVICE, n_in samples.  out: DEVICE, room for out_cap samples.  Enqueues on the handle's stream, reads nothing back
 * and does not wait.  Refused with gr4pm_last_error set, *n_out = 0, nothing enqueued and the handle unchanged: a NULL in
 * with n_in > 0, a NULL out when the call delivers samples (GR4PM_ERR_INVALID); n_in > 2^40 or fewer than the samples of
 * room (GR4PM_ERR_OVERFLOW). */
gr4pm_status gr4pm_fft_filter_process(gr4pm_fft_filter* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_cap,
                                      size_t* n_out);
/* The same for integer IQ in (GR4PM_IQ_SC16 / SC8 / CU8; scale 0: the format's default), gr4pm_ddc_process_iq's contract
 * for the input side: gr4pm_fft_filter_process on gr4pm_iq_unpack(in) bit for bit; calls of any format mix on one handle.
 * An unknown format is refused with GR4PM_ERR_INVALID before anything is enqueued. */
gr4pm_status gr4pm_fft_filter_process_iq(gr4pm_fft_filter* h, const void* in, int format, float scale, size_t n_in, gr4pm_c64* out,
                                         size_t out_cap, size_t* n_out);
/* The `pending` samples still owed: the last segment run over zeros, its first `pending` kept samples to out.  Leaves the
 * handle as gr4pm_fft_filter_reset does, so the samples out equal the samples in.  Refused with the handle unchanged: fewer
 * than `pending` samples of room (GR4PM_ERR_OVERFLOW), a NULL out with samples owed (GR4PM_ERR_INVALID). */
gr4pm_status gr4pm_fft_filter_flush(gr4pm_fft_filter* h, gr4pm_c64* out, size_t out_cap, size_t* n_out);

/* Host only: complex taps that stop (GR4PM_BAND_STOP) or pass (GR4PM_BAND_PASS) the given bands.  bands: n_bands pairs
 * (centre, width) in cycles per sample; a band may wrap across +-0.5; bands that overlap or touch are merged on the circle.
 * n_taps odd, c = (n_taps - 1) / 2; Kaiser window w with beta from attenuation_db = A (A > 50: 0.1102 (A - 8.7); A >= 21:
 * 0.5842 (A - 21)^0.4 + 0.07886 (A - 21); else 0); per merged band [f_lo, f_hi]
 *     g_b(m) = (e^{2 pi j f_hi m} - e^{2 pi j f_lo m}) / (2 pi j m),   g_b(0) = f_hi - f_lo
 *     pass: h[t] = w[t] sum_b g_b(t - c);   stop: h[t] = w[t] (delta[t - c] - sum_b g_b(t - c))
 * in double, each component rounded to float once.  The filter delays by c samples; its transition width is
 * (A - 7.95) / (14.36 (n_taps - 1)) cycles per sample.  Refused with GR4PM_ERR_INVALID and a text: a NaN or infinite
 * input, a width <= 0 or >= 1, an even n_taps or n_taps < 3, A <= 8, bands that merge to the whole circle, an unknown mode. */
enum { GR4PM_BAND_STOP = 0, GR4PM_BAND_PASS = 1 };
gr4pm_status gr4pm_band_filter_taps(const double* bands, size_t n_bands, int mode, size_t n_taps, double attenuation_db,
                                    gr4pm_c64* taps_out);

#ifdef __cplusplus
}
#endif
#endif /* GR4PM_HIP_H */
