// packet_control_blocks.hip -- SyncwordWipeoff, SyncwordDetectionFilter, PayloadMetadataInsert, SyncwordRemove,
// ConstellationLLRDecoder: the blocks whose host side is hostlogic/packet_control.hpp and hostlogic/sdf_gate.hpp, with
// their small kernels.  (Conventions of the stream blocks: stream_blocks.hpp.)
#include "stream_blocks.hpp"
#include "hostlogic/packet_control.hpp"
#include "hostlogic/sdf_gate.hpp"

namespace gr4pm {
namespace {

// =====================================================================================
// SyncwordWipeoff (syncword_wipeoff.hpp:66-82): copy, then x[pos] *= syncword[pos] on spans
// =====================================================================================
using hostlogic::WipeSpan; // hostlogic/packet_control.hpp
__global__ void k_wipe(const WipeSpan* __restrict__ spans, const float* __restrict__ syncword,
                       const cf* in, cf* out) // may be the same buffer
{
    const WipeSpan w = spans[blockIdx.x];
    for (unsigned i = threadIdx.x; i < w.len; i += blockDim.x)
        out[w.start + i] = fmulc(syncword[w.first + i], in[w.start + i]);
}

template <typename T>
__global__ void k_copy(const T* __restrict__ in, T* __restrict__ out, size_t n)
{
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * blockDim.x)
        out[i] = in[i];
}

} // namespace
} // namespace gr4pm

using namespace gr4pm;

// ------------------------------------------------------------------------ SyncwordWipeoff
struct gr4pm_syncword_wipeoff : gr4pm::hostlogic::WipeState { // the state machine: hostlogic/packet_control.hpp
    std::vector<float> syncword;
    hipStream_t stream;
    DevBuf<float> d_syncword;
    DevBuf<WipeSpan> spans;
};
using hostlogic::wipe_replay;

extern "C" {

gr4pm_status gr4pm_syncword_wipeoff_create(const gr4pm_syncword_wipeoff_params* p,
                                           gr4pm_syncword_wipeoff** out)
try {
    if (!p || !out || !p->syncword || p->n_syncword == 0) return GR4PM_ERR_INVALID;
    *out = nullptr;
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_syncword_wipeoff> h(new (std::nothrow) gr4pm_syncword_wipeoff);
    if (!h) return GR4PM_ERR_NOMEM;
    h->syncword.assign(p->syncword, p->syncword + p->n_syncword);
    h->syncword_size = p->n_syncword;
    h->stream = static_cast<hipStream_t>(p->stream);
    GR4PM_TRY(h->d_syncword.alloc(p->n_syncword));
    GR4PM_TRY(h->d_syncword.upload(h->syncword.data(), h->syncword.size(), h->stream));
    return finish_create(h, out, "syncword_wipeoff");
}
GR4PM_ABI_CATCH
void gr4pm_syncword_wipeoff_destroy(gr4pm_syncword_wipeoff* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_syncword_wipeoff_reset(gr4pm_syncword_wipeoff* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    h->in_syncword = false;
    h->position = 0;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_syncword_wipeoff_process(gr4pm_syncword_wipeoff* h, const gr4pm_c64* in, size_t n,
                                            gr4pm_c64* out, const gr4pm_tag* tags, size_t n_tags)
try {
    if (!h) return GR4PM_ERR_INVALID;
    if (n == 0) return GR4PM_OK;
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    std::vector<WipeSpan> spans;
    wipe_replay(*h, n, tags, n_tags, 0, spans);
    hipStream_t s = h->stream;
    if (in != out) // in place: only the syncword spans are touched
        hipLaunchKernelGGL(k_copy<cf>, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s,
                           reinterpret_cast<const cf*>(in), reinterpret_cast<cf*>(out), n);
    if (!spans.empty()) {
        GR4PM_TRY(upload_vec(h->spans, spans, s));
        hipLaunchKernelGGL(k_wipe, dim3(static_cast<unsigned>(spans.size())), dim3(64), 0, s, h->spans.p,
                           h->d_syncword.p, reinterpret_cast<const cf*>(in), reinterpret_cast<cf*>(out));
    }
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(final_sync(s));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_syncword_wipeoff_process_channels(gr4pm_syncword_wipeoff* const* h, size_t n_channels,
                                                     gr4pm_c64* buf, size_t stride, const size_t* n,
                                                     const gr4pm_tag* const* tags, const size_t* n_tags)
try {
    if (!h || n_channels == 0 || !n || !tags || !n_tags) return GR4PM_ERR_INVALID;
    if (!buf) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    std::vector<WipeSpan> spans;
    for (size_t c = 0; c < n_channels; ++c) {
        if (!h[c] || h[c]->syncword != h[0]->syncword || n[c] > stride) {
            set_error("a launch that spans channels needs wipe-off blocks of one syncword and n <= stride");
            return GR4PM_ERR_INVALID;
        }
        wipe_replay(*h[c], n[c], tags[c], n_tags[c], c * stride, spans);
    }
    hipStream_t s = h[0]->stream;
    if (!spans.empty()) {
        GR4PM_TRY(upload_vec(h[0]->spans, spans, s));
        hipLaunchKernelGGL(k_wipe, dim3(static_cast<unsigned>(spans.size())), dim3(64), 0, s, h[0]->spans.p,
                           h[0]->d_syncword.p, reinterpret_cast<const cf*>(buf), reinterpret_cast<cf*>(buf));
    }
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(final_sync(s));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"

// ------------------------------------------------------------------ SyncwordDetectionFilter
// the state machine itself: hostlogic/sdf_gate.hpp (no HIP; also built with sanitizers by tests/hostlogic/)
struct gr4pm_syncword_detection_filter : gr4pm::hostlogic::SdfState {
    hipStream_t stream = nullptr;
};

extern "C" {

gr4pm_status gr4pm_syncword_detection_filter_create(const gr4pm_syncword_detection_filter_params* p,
                                                    gr4pm_syncword_detection_filter** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_syncword_detection_filter> h(new (std::nothrow) gr4pm_syncword_detection_filter);
    if (!h) return GR4PM_ERR_NOMEM;
    h->sps = p->samples_per_symbol;
    h->syncword_size = p->syncword_size;
    h->header_size = p->header_size;
    h->stream = static_cast<hipStream_t>(p->stream);
    *out = h.release(); // (nothing was queued on the stream: nothing to wait for)
    return GR4PM_OK;
}
GR4PM_ABI_CATCH
void gr4pm_syncword_detection_filter_destroy(gr4pm_syncword_detection_filter* h)
try {
    delete h;
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_syncword_detection_filter_reset(gr4pm_syncword_detection_filter* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    h->in_packet = false; // start(), :52
    h->gate_in_packet = false;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_syncword_detection_filter_process(gr4pm_syncword_detection_filter* h, const gr4pm_c64* in,
                                                     size_t n_in, gr4pm_c64* out, size_t out_cap,
                                                     int head_tag_flags, const gr4pm_header_msg* headers,
                                                     size_t n_headers, size_t n_ignored, size_t* consumed_,
                                                     size_t* headers_consumed, size_t* ignored_consumed,
                                                     int* tag_out_flags)
try {
    if (!h || !consumed_ || !headers_consumed || !ignored_consumed || !tag_out_flags) return GR4PM_ERR_INVALID;
    gr4pm::hostlogic::CopySpan runs[2];
    int n_runs = 0;
    GR4PM_TRY(gr4pm::hostlogic::sdf_process_plan(*h, n_in, out_cap, head_tag_flags, headers, n_headers, n_ignored,
                                                 consumed_, headers_consumed, ignored_consumed, tag_out_flags, runs,
                                                 &n_runs));
    for (int r = 0; r < n_runs; ++r)
        GR4PM_HIP_TRY(hipMemcpyAsync(out + runs[r].dst, in + runs[r].src, runs[r].len * sizeof(gr4pm_c64),
                                     hipMemcpyDeviceToDevice, h->stream));
    GR4PM_HIP_TRY(hipStreamSynchronize(h->stream));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"

extern "C" gr4pm_status gr4pm_syncword_detection_filter_gate(gr4pm_syncword_detection_filter* h,
                                                             const uint64_t* tag_index, size_t n_tags,
                                                             const gr4pm_header_msg* headers, size_t n_headers,
                                                             int headers_per_tag, uint8_t* accepted,
                                                             size_t* headers_used)
try {
    if (!h || !accepted || !headers_used) return GR4PM_ERR_INVALID;
    return gr4pm::hostlogic::sdf_gate(*h, tag_index, n_tags, headers, n_headers, headers_per_tag, accepted, headers_used);
}
GR4PM_ABI_CATCH

extern "C" gr4pm_status gr4pm_syncword_detection_filter_gate_resolve(gr4pm_syncword_detection_filter* h,
                                                                     const gr4pm_header_msg* msg)
try {
    if (!h || !msg) return GR4PM_ERR_INVALID;
    return gr4pm::hostlogic::sdf_gate_resolve(*h, *msg);
}
GR4PM_ABI_CATCH

// =====================================================================================
// Symbol-rate control blocks behind SyncwordWipeoff (include/gr4pm_hip.h).
// The per-item work of PayloadMetadataInsert and SyncwordRemove is a gather of item spans;
// which spans is decided by a host replay of the blocks' state machines over the tags.
// =====================================================================================
namespace gr4pm {
namespace {

using hostlogic::CopySpan; // hostlogic/base.hpp
// grid (x, n_spans): the blocks of a row walk their span with coalesced 8-byte accesses
__global__ __launch_bounds__(256) void k_gather_spans(const CopySpan* __restrict__ spans, const cf* __restrict__ in,
                                                      cf* __restrict__ out)
{
    const CopySpan sp = spans[blockIdx.y];
    const cf* src = in + sp.src;
    cf* dst = out + sp.dst;
    for (unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < sp.len;
         i += static_cast<unsigned long long>(gridDim.x) * blockDim.x)
        dst[i] = src[i];
}
gr4pm_status launch_gather(hipStream_t s, DevBuf<CopySpan>& buf, const std::vector<CopySpan>& spans, const cf* in,
                           cf* out)
{
    if (spans.empty()) return GR4PM_OK;
    GR4PM_TRY(upload_vec(buf, spans, s));
    unsigned long long longest = 0;
    for (const auto& sp : spans) longest = std::max(longest, sp.len);
    const unsigned gx = static_cast<unsigned>(std::min<unsigned long long>((longest + 2047) / 2048, 1024));
    for (size_t first = 0; first < spans.size(); first += 65535) { // gridDim.y limit
        const unsigned rows = static_cast<unsigned>(std::min<size_t>(65535, spans.size() - first));
        hipLaunchKernelGGL(k_gather_spans, dim3(std::max(gx, 1u), rows), dim3(256), 0, s, buf.p + first, in, out);
    }
    GR4PM_HIP_TRY(hipGetLastError());
    return GR4PM_OK;
}

// LLR mapping of one run of symbols with one constellation: BPSK scale * re, QPSK
// (scale * re, scale * im) = a scaled copy of the interleaved floats
using hostlogic::LlrRun; // hostlogic/packet_control.hpp
__global__ __launch_bounds__(256) void k_llr(const LlrRun* __restrict__ runs, float scale,
                                             const float* __restrict__ in, float* __restrict__ out)
{
    const LlrRun r = runs[blockIdx.y];
    const float* src = in + 2 * r.in0;
    float* dst = out + r.out0;
    for (unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < r.n_out;
         i += static_cast<unsigned long long>(gridDim.x) * blockDim.x)
        dst[i] = scale * src[r.qpsk ? i : 2 * i]; // constellation_llr_decoder.hpp:106-116
}

} // namespace
} // namespace gr4pm

struct gr4pm_payload_metadata_insert : gr4pm::hostlogic::PmiState {
    hipStream_t stream = nullptr;
    DevBuf<gr4pm::hostlogic::CopySpan> spans;
};
struct gr4pm_syncword_remove : gr4pm::hostlogic::SrState {
    hipStream_t stream = nullptr;
    DevBuf<gr4pm::hostlogic::CopySpan> spans;
};
struct gr4pm_constellation_llr_decoder : gr4pm::hostlogic::LlrState { // the constellation follows the tags: hostlogic/packet_control.hpp
    float noise_sigma, scale;
    hipStream_t stream;
    DevBuf<LlrRun> runs;
};

using gr4pm::hostlogic::llr_runs;
// (library-internal) PayloadMetadataInsert::processBulk's host half: the state machine over the tags (hostlogic/packet_control.hpp)
gr4pm_status gr4pm::payload_metadata_insert_plan(gr4pm_payload_metadata_insert* h, size_t n_in, size_t out_cap,
                                                 const gr4pm_tag* tags_in, size_t n_tags_in, const gr4pm_header_msg* headers,
                                                 size_t n_headers, int headers_per_tag, gr4pm_packet_tag* tags_out, size_t tags_cap,
                                                 size_t* n_tags_out, size_t* consumed, size_t* produced, size_t* headers_used,
                                                 size_t* ignored_syncwords, std::vector<hostlogic::CopySpan>& spans)
{
    if (!h || !n_tags_out || !consumed || !produced || !headers_used || !ignored_syncwords) return GR4PM_ERR_INVALID;
    *n_tags_out = *consumed = *produced = *headers_used = *ignored_syncwords = 0;
    spans.clear();
    if (headers_per_tag && n_headers != n_tags_in) {
        set_error("headers_per_tag needs one message per tag (%zu != %zu)", n_headers, n_tags_in);
        return GR4PM_ERR_INVALID;
    }
    if (n_in == 0) return GR4PM_OK;
    hostlogic::PmiReplay rp;
    GR4PM_TRY(hostlogic::pmi_replay(*h, n_in, out_cap, tags_in, n_tags_in, headers, n_headers, headers_per_tag, tags_out,
                                    tags_cap, rp));
    spans.swap(rp.spans);
    *n_tags_out = rp.n_pub;
    *consumed = rp.consumed;
    *produced = rp.produced;
    *headers_used = rp.headers_used;
    *ignored_syncwords = rp.ignored;
    if (rp.tag_overflow) {
        set_error("tags_cap too small");
        return GR4PM_ERR_OVERFLOW;
    }
    return GR4PM_OK;
}
// (library-internal: csrc/packet_receiver.hip, the packets_only receiver) the host halves alone: state, tags, spans
gr4pm_status gr4pm::syncword_remove_plan(gr4pm_syncword_remove* h, size_t n, const gr4pm_packet_tag* tags_in, size_t n_tags_in,
                                         gr4pm_packet_tag* tags_out, size_t tags_cap, size_t* n_tags_out, size_t* produced,
                                         std::vector<hostlogic::CopySpan>& spans)
{
    if (!h || !produced) return GR4PM_ERR_INVALID;
    hostlogic::SrReplay rp; // the state machine: hostlogic/packet_control.hpp
    hostlogic::sr_replay(*h, n, tags_in, n_tags_in, tags_out, tags_cap, rp);
    spans.swap(rp.spans);
    *produced = rp.produced;
    if (n_tags_out) *n_tags_out = rp.n_pub;
    if (rp.tag_overflow) {
        set_error("tags_cap too small");
        return GR4PM_ERR_OVERFLOW;
    }
    return GR4PM_OK;
}
gr4pm_status gr4pm::llr_decoder_plan(gr4pm_constellation_llr_decoder* h, size_t n, const gr4pm_packet_tag* tags_in,
                                     size_t n_tags_in, gr4pm_packet_tag* tags_out, size_t tags_cap, size_t* n_tags_out,
                                     size_t* produced, bool* all_qpsk, float* scale)
{
    if (!h || !produced || !all_qpsk || !scale) return GR4PM_ERR_INVALID;
    std::vector<LlrRun> runs;
    *produced = 0;
    if (n_tags_out) *n_tags_out = 0;
    const gr4pm_status st = llr_runs(*h, n, static_cast<size_t>(-1), tags_in, n_tags_in, tags_out, tags_cap, n_tags_out, produced, runs);
    *all_qpsk = true;
    for (const auto& r : runs) *all_qpsk = *all_qpsk && r.qpsk;
    *scale = h->scale;
    return st;
}

extern "C" {

gr4pm_status gr4pm_payload_metadata_insert_create(const gr4pm_payload_metadata_insert_params* p,
                                                  gr4pm_payload_metadata_insert** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_payload_metadata_insert> h(new (std::nothrow) gr4pm_payload_metadata_insert);
    if (!h) return GR4PM_ERR_NOMEM;
    h->syncword_size = p->syncword_size;
    h->header_size = p->header_size;
    h->syncword_bw = p->syncword_costas_loop_bandwidth;
    h->header_bw = p->header_costas_loop_bandwidth;
    h->payload_bw = p->payload_costas_loop_bandwidth;
    h->stream = static_cast<hipStream_t>(p->stream);
    *out = h.release(); // (nothing was queued on the stream: nothing to wait for)
    return GR4PM_OK;
}
GR4PM_ABI_CATCH
void gr4pm_payload_metadata_insert_destroy(gr4pm_payload_metadata_insert* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_payload_metadata_insert_reset(gr4pm_payload_metadata_insert* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    h->in_packet = false; // start(), :71-75
    h->position = 0;
    h->has_held = false;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_payload_metadata_insert_process(
    gr4pm_payload_metadata_insert* h, const gr4pm_c64* in, size_t n_in, gr4pm_c64* out, size_t out_cap,
    const gr4pm_tag* tags_in, size_t n_tags_in, const gr4pm_header_msg* headers, size_t n_headers,
    int headers_per_tag, gr4pm_packet_tag* tags_out, size_t tags_cap, size_t* n_tags_out, size_t* consumed,
    size_t* produced, size_t* headers_used, size_t* ignored_syncwords)
try {
    if (!h || !n_tags_out || !consumed || !produced || !headers_used || !ignored_syncwords) return GR4PM_ERR_INVALID;
    *n_tags_out = *consumed = *produced = *headers_used = *ignored_syncwords = 0;
    if (n_in && (!in || !out)) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    std::vector<CopySpan> spans;
    const gr4pm_status st = gr4pm::payload_metadata_insert_plan(h, n_in, out_cap, tags_in, n_tags_in, headers, n_headers,
                                                                headers_per_tag, tags_out, tags_cap, n_tags_out, consumed,
                                                                produced, headers_used, ignored_syncwords, spans);
    if (st != GR4PM_OK && st != GR4PM_ERR_OVERFLOW) return st;
    GR4PM_TRY(launch_gather(h->stream, h->spans, spans, reinterpret_cast<const cf*>(in), reinterpret_cast<cf*>(out)));
    GR4PM_HIP_TRY(final_sync(h->stream));
    return st;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_payload_metadata_insert_resolve(gr4pm_payload_metadata_insert* h, const gr4pm_header_msg* msg)
try {
    if (!h || !msg) return GR4PM_ERR_INVALID;
    if (h->in_packet && !h->has_held) {
        h->held = *msg;
        h->has_held = true;
    }
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_syncword_remove_create(const gr4pm_syncword_remove_params* p, gr4pm_syncword_remove** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_syncword_remove> h(new (std::nothrow) gr4pm_syncword_remove);
    if (!h) return GR4PM_ERR_NOMEM;
    h->syncword_size = p->syncword_size;
    h->stream = static_cast<hipStream_t>(p->stream);
    *out = h.release(); // (nothing was queued on the stream: nothing to wait for)
    return GR4PM_OK;
}
GR4PM_ABI_CATCH
void gr4pm_syncword_remove_destroy(gr4pm_syncword_remove* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_syncword_remove_reset(gr4pm_syncword_remove* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    h->in_syncword = false;
    h->position = 0;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH
gr4pm_status gr4pm_syncword_remove_process(gr4pm_syncword_remove* h, const gr4pm_c64* in, size_t n, gr4pm_c64* out,
                                           const gr4pm_packet_tag* tags_in, size_t n_tags_in,
                                           gr4pm_packet_tag* tags_out, size_t tags_cap, size_t* n_tags_out,
                                           size_t* produced)
try {
    if (!h || !produced) return GR4PM_ERR_INVALID;
    *produced = 0;
    if (n_tags_out) *n_tags_out = 0;
    if (n == 0) return GR4PM_OK;
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    std::vector<CopySpan> spans;
    const gr4pm_status st = gr4pm::syncword_remove_plan(h, n, tags_in, n_tags_in, tags_out, tags_cap, n_tags_out, produced, spans);
    if (st != GR4PM_OK && st != GR4PM_ERR_OVERFLOW) return st;
    GR4PM_TRY(launch_gather(h->stream, h->spans, spans, reinterpret_cast<const cf*>(in), reinterpret_cast<cf*>(out)));
    GR4PM_HIP_TRY(final_sync(h->stream));
    return st;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_constellation_llr_decoder_create(const gr4pm_constellation_llr_decoder_params* p,
                                                    gr4pm_constellation_llr_decoder** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    if (p->constellation != 1 && p->constellation != 2) { // :72-74
        set_error("constellation %d not supported", p->constellation);
        return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_constellation_llr_decoder> h(new (std::nothrow) gr4pm_constellation_llr_decoder);
    if (!h) return GR4PM_ERR_NOMEM;
    h->noise_sigma = p->noise_sigma;
    h->scale = 2.0f / (p->noise_sigma * p->noise_sigma); // :77
    h->constellation = p->constellation;
    h->stream = static_cast<hipStream_t>(p->stream);
    *out = h.release(); // (nothing was queued on the stream: nothing to wait for)
    return GR4PM_OK;
}
GR4PM_ABI_CATCH
void gr4pm_constellation_llr_decoder_destroy(gr4pm_constellation_llr_decoder* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID
gr4pm_status gr4pm_constellation_llr_decoder_process(gr4pm_constellation_llr_decoder* h, const gr4pm_c64* in,
                                                     size_t n, float* out, size_t out_cap,
                                                     const gr4pm_packet_tag* tags_in, size_t n_tags_in,
                                                     gr4pm_packet_tag* tags_out, size_t tags_cap,
                                                     size_t* n_tags_out, size_t* produced)
try {
    if (!h || !produced) return GR4PM_ERR_INVALID;
    *produced = 0;
    if (n_tags_out) *n_tags_out = 0;
    if (n == 0) return GR4PM_OK;
    if (!in || !out) {
        set_error("null sample pointer");
        return GR4PM_ERR_INVALID;
    }
    std::vector<LlrRun> runs;
    const gr4pm_status st = llr_runs(*h, n, out_cap, tags_in, n_tags_in, tags_out, tags_cap, n_tags_out, produced, runs);
    if (st != GR4PM_OK && st != GR4PM_ERR_OVERFLOW) return st;
    GR4PM_TRY(upload_vec(h->runs, runs, h->stream));
    unsigned long long longest = 0;
    for (const auto& r : runs) longest = std::max(longest, r.n_out);
    const unsigned gx = static_cast<unsigned>(std::min<unsigned long long>((longest + 2047) / 2048, 1024));
    for (size_t first = 0; first < runs.size(); first += 65535) {
        const unsigned rows = static_cast<unsigned>(std::min<size_t>(65535, runs.size() - first));
        hipLaunchKernelGGL(k_llr, dim3(std::max(gx, 1u), rows), dim3(256), 0, h->stream, h->runs.p + first, h->scale,
                           reinterpret_cast<const float*>(in), out);
    }
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(final_sync(h->stream));
    return st;
}
GR4PM_ABI_CATCH

} // extern "C"
