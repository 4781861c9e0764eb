// packet_transmitter.hip -- PacketTransmitterPdu (packet_transmitter_pdu.hpp:40-355): payload bytes to shaped IQ
// bursts (or one continuous stream) in two launches per call.
//
//   k_tx_prepass  one wave per packet: CRC-32 (crc_append.hpp), the header (header_formatter.hpp:110-113) and its
//                 LDPC(128,32) code word (header_fec_encoder.hpp:60-107), the 18 ramp-down bits of the burst from the
//                 degree-32 GLFSR jumped ahead on the device, and the tile -> first burst table of the sample kernel.
//   k_tx_samples  one workgroup per tile of kTxTile output samples: the symbols the tile needs (filter history
//                 included) are built in LDS burst by burst, then every lane forms its samples with the reference's
//                 polyphase MAC order (interpolating_fir_filter.hpp:96,158-165), applies the burst shaper's ramps
//                 (burst_shaper.hpp:98-124) and writes the tile, gaps as zeros, with 16-byte stores.
//   k_tx_carry    stream mode: the last symbols of the call become the filter history of the next one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"

using namespace gr4pm;

namespace {

constexpr unsigned kTxThreads = 256;
constexpr unsigned kTxTile = 4096;                       // output samples per workgroup
constexpr unsigned kTxPairs = kTxTile / (2 * kTxThreads); // 16-byte stores per lane
constexpr unsigned kTxMaxSps = 64;
constexpr unsigned kSyncSymbols = 64, kHeaderSymbols = 128, kRampSymbols = 9, kFlushSymbols = 11;
constexpr unsigned long long kSyncword = 0x034776C7272895B0ull; // packet_transmitter_pdu.hpp:161-175, first bit = MSB
constexpr uint32_t kCrcPoly = 0xEDB88320u;                      // 0x4C11DB7 reflected
constexpr uint32_t kGlfsrMask = 0x80000057u;                    // glfsr_source.hpp:72, degree 32
constexpr unsigned kMaxPacketLength = 65535;                    // header_formatter.hpp:102-106

struct TxPacket {
    unsigned long long in_off;  // first payload byte in the input
    unsigned long long out_off; // first output sample of the burst (behind its gap)
    unsigned n_samples;         // samples of the burst
    unsigned len;               // payload bytes
    unsigned type;              // 0 USER_DATA, 1 IDLE
    unsigned pad;
};
struct TxDerived {
    uint32_t hdr[4]; // info word, then the 96 parity bits, each word MSB first
    uint32_t crc;
    uint32_t ramp; // bit i = the burst's i-th ramp-down bit
    uint32_t pad[2];
};
static_assert(sizeof(TxPacket) == 32 && sizeof(TxDerived) == 32, "one 32-byte load each");

// a(x) b(x) mod P in the reflected representation (bit 31 = x^0), as zlib's multmodp
__host__ __device__ inline uint32_t multmodp(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
__host__ __device__ inline uint32_t glfsr_step(uint32_t r) { return (r >> 1) ^ ((r & 1) ? kGlfsrMask : 0u); }
// M s over GF(2), M given by its 32 columns
__host__ __device__ inline uint32_t gf2_apply(const uint32_t* col, uint32_t s)
{
    uint32_t r = 0;
    for (unsigned i = 0; i < 32; ++i)
        if ((s >> i) & 1u) r ^= col[i];
    return r;
}
// the GLFSR register after `n` bursts (18 steps each): jump[k] = M18^(2^k)
__host__ __device__ inline uint32_t glfsr_jump(const uint32_t* jump, uint32_t s, unsigned long long n)
{
    for (unsigned k = 0; n; ++k, n >>= 1)
        if (n & 1) s = gf2_apply(jump + 32 * k, s);
    return s;
}

// consts: [0, 256) the reflected CRC-32 byte table, [256, 288) x^(2^k) mod P, [288, 384) the LDPC generator rows
constexpr unsigned kConstCrc = 0, kConstX2n = 256, kConstGen = 288, kConstWords = 384;

__global__ __launch_bounds__(kTxThreads) void k_tx_prepass(const TxPacket* __restrict__ pk, unsigned n_packets,
                                                           const uint8_t* __restrict__ payload,
                                                           const uint32_t* __restrict__ consts,
                                                           const uint32_t* __restrict__ jump, uint32_t glfsr0,
                                                           unsigned* __restrict__ tile_first, TxDerived* __restrict__ dv)
{
    __shared__ uint32_t T[256];
    for (unsigned i = threadIdx.x; i < 256; i += kTxThreads) T[i] = consts[kConstCrc + i];
    __syncthreads();
    const unsigned lane = threadIdx.x & 63;
    const unsigned p = blockIdx.x * (kTxThreads / 64) + threadIdx.x / 64;
    if (p >= n_packets) return;
    const TxPacket q = pk[p];
    // CRC-32: lane i runs over its own chunk from a zero register (lane 0 from the initial value); the register is
    // linear in what it starts from, so each lane's part is shifted over the bytes behind its chunk and XORed
    const unsigned C = (q.len + 63) / 64;
    const unsigned lo = lane * C, hi = min(lo + C, q.len);
    uint32_t part = 0;
    if (lo < q.len) {
        const uint8_t* d = payload + q.in_off;
        uint32_t reg = lane == 0 ? 0xFFFFFFFFu : 0u;
        for (unsigned k = lo; k < hi; ++k) reg = T[(reg ^ d[k]) & 0xffu] ^ (reg >> 8);
        uint32_t shift = 1u << 31; // x^(8 (len - hi)) mod P
        unsigned n = q.len - hi;
        for (unsigned k = 3; n; ++k, n >>= 1)
            if (n & 1) shift = multmodp(consts[kConstX2n + k], shift);
        part = multmodp(shift, reg);
    }
    for (unsigned off = 32; off; off >>= 1) part ^= __shfl_xor(part, off, 64);
    const uint32_t info = ((q.len >> 8) & 0xffu) << 24 | (q.len & 0xffu) << 16 | (q.type ? 1u : 0u) << 8 | 0x55u;
    // parity bit j = <info, generator row j>: lanes 0..63 the first 64, lanes 0..31 the remaining 32
    const bool p0 = __popc(info & consts[kConstGen + lane]) & 1;
    const bool p1 = lane < 32 && (__popc(info & consts[kConstGen + 64 + (lane & 31)]) & 1);
    const unsigned long long b0 = __ballot(p0), b1 = __ballot(p1);
    if (lane == 0) {
        TxDerived o;
        o.hdr[0] = info;
        o.hdr[1] = __brev(static_cast<uint32_t>(b0));
        o.hdr[2] = __brev(static_cast<uint32_t>(b0 >> 32));
        o.hdr[3] = __brev(static_cast<uint32_t>(b1));
        o.crc = part ^ 0xFFFFFFFFu;
        uint32_t r = glfsr_jump(jump, glfsr0, p), bits = 0;
        for (unsigned i = 0; i < 2 * kRampSymbols; ++i) { // glfsr_source.hpp:93-101
            bits |= (r & 1u) << i;
            r = glfsr_step(r);
        }
        o.ramp = bits;
        o.pad[0] = o.pad[1] = 0;
        dv[p] = o;
    }
    // tiles whose first sample lies in this burst or in the gap in front of it start their search here
    const unsigned long long prev_end = p ? pk[p - 1].out_off + pk[p - 1].n_samples : 0ull;
    const unsigned long long end = q.out_off + q.n_samples;
    for (unsigned long long t = (prev_end + kTxTile - 1) / kTxTile + lane; t * kTxTile < end; t += 64)
        tile_first[t] = p;
}

struct TxSym {
    const TxPacket* pk;
    const TxDerived* dv;
    const uint8_t* payload;
    const uint8_t* scr; // scrambler output bits, packed MSB first: restarted at the header's first bit
    float qa;           // sqrt(2)/2, packet_transmitter_pdu.hpp:131
};
__device__ inline unsigned tx_symbols(unsigned len, bool stream)
{
    return kSyncSymbols + kHeaderSymbols + 4 * (len + 4) + (stream ? 0 : kRampSymbols + kFlushSymbols);
}
// symbol n (0 <= n < tx_symbols) of packet b
__device__ inline float2 tx_symbol(const TxSym& a, const TxPacket& q, const TxDerived& dv, unsigned n)
{
    if (n < kSyncSymbols) return make_float2((kSyncword >> (63 - n)) & 1 ? -1.f : 1.f, 0.f);
    unsigned k = n - kSyncSymbols;
    unsigned idx;
    const unsigned body = 4 * (32 + q.len + 4);
    if (k < body) {
        const unsigned B = k >> 2;
        unsigned byte;
        if (B < 32) { // (selects: an indexed load from a register array would go through scratch)
            const unsigned w = (B & 15) >> 2;
            byte = (w == 0 ? dv.hdr[0] : w == 1 ? dv.hdr[1] : w == 2 ? dv.hdr[2] : dv.hdr[3]) >> (8 * (3 - (B & 3)));
        }
        else if (B < 32 + q.len)
            byte = a.payload[q.in_off + B - 32];
        else
            byte = dv.crc >> (8 * (3 - (B - 32 - q.len))); // big-endian, crc_append.hpp:176-179
        idx = ((byte ^ a.scr[B]) >> (6 - 2 * (k & 3))) & 3u;
    } else {
        k -= body;
        if (k >= kRampSymbols) return make_float2(0.f, 0.f);
        idx = ((dv.ramp >> (2 * k)) & 1u) << 1 | ((dv.ramp >> (2 * k + 1)) & 1u);
    }
    return make_float2(idx & 2 ? -a.qa : a.qa, idx & 1 ? -a.qa : a.qa); // {a,a},{a,-a},{-a,a},{-a,-a}
}

// LDS: the symbols of the current burst segment (kTxTile / sps + stride + 1 of them), then the taps [sps][stride]
// (zero-padded arms), the leading ramp (8 sps) and the trailing ramp (11 sps)
inline size_t tx_smem(unsigned sps, unsigned stride)
{
    return (kTxTile / sps + stride + 1) * sizeof(float2) + (sps * stride + 19 * sps) * sizeof(float);
}

template <bool STREAM>
__global__ __launch_bounds__(kTxThreads) void k_tx_samples(TxSym a, unsigned n_packets,
                                                           const unsigned* __restrict__ tile_first,
                                                           const float* __restrict__ taps, unsigned sps,
                                                           unsigned stride, const float2* __restrict__ hist,
                                                           unsigned long long n_out, float2* __restrict__ out)
{
    extern __shared__ float4 s_tx[];
    float2* s_sym = reinterpret_cast<float2*>(s_tx);
    float* s_taps = reinterpret_cast<float*>(s_sym + kTxTile / sps + stride + 1);
    const unsigned n_taps = sps * stride + 19 * sps;
    for (unsigned i = threadIdx.x; i < n_taps; i += kTxThreads) s_taps[i] = taps[i];
    const float* s_lead = s_taps + sps * stride;
    const float* s_trail = s_lead + 8 * sps;
    const unsigned n_lead = 8 * sps, n_trail = 11 * sps;

    const unsigned long long S0 = static_cast<unsigned long long>(blockIdx.x) * kTxTile;
    const unsigned long long S1 = min(S0 + kTxTile, n_out);
    float2 r[2 * kTxPairs];
    for (unsigned k = 0; k < 2 * kTxPairs; ++k) r[k] = make_float2(0.f, 0.f); // gaps
    for (unsigned b = tile_first[blockIdx.x]; b < n_packets; ++b) {
        const TxPacket q = a.pk[b];
        if (q.out_off >= S1) break;
        const unsigned long long qe = q.out_off + q.n_samples;
        if (qe <= S0) continue;
        const TxDerived dv = a.dv[b];
        const unsigned t_a = static_cast<unsigned>(max(S0, q.out_off) - q.out_off);
        const unsigned t_e = static_cast<unsigned>(min(S1, qe) - q.out_off);
        const int n_lo = static_cast<int>(t_a / sps) - static_cast<int>(stride - 1);
        const int n_hi = static_cast<int>((t_e - 1) / sps);
        __syncthreads(); // the segment before is no longer read (and the taps are staged)
        for (int i = threadIdx.x; i <= n_hi - n_lo; i += kTxThreads) {
            const int n = n_lo + i;
            float2 v;
            if (n >= 0) {
                v = tx_symbol(a, q, dv, static_cast<unsigned>(n));
            } else if (!STREAM) {
                v = make_float2(0.f, 0.f); // the 11 flush symbols of the burst before / the silent filter
            } else if (b == 0) {
                v = hist[static_cast<int>(stride - 1) + n];
            } else {
                const TxPacket pq = a.pk[b - 1];
                v = tx_symbol(a, pq, a.dv[b - 1], tx_symbols(pq.len, true) + n);
            }
            s_sym[i] = v;
        }
        __syncthreads();
#pragma unroll
        for (unsigned k = 0; k < kTxPairs; ++k) {
#pragma unroll
            for (unsigned e = 0; e < 2; ++e) {
                const unsigned long long s = S0 + 2ull * (k * kTxThreads + threadIdx.x) + e;
                if (s < q.out_off || s >= qe || s >= S1) continue;
                const unsigned t = static_cast<unsigned>(s - q.out_off);
                const unsigned n = t / sps, j = t - n * sps;
                const float2* x = s_sym + (static_cast<int>(n) - n_lo);
                const float* arm = s_taps + j * stride;
                float2 acc = make_float2(0.f, 0.f); // padded arms add +-0 products: no bit changes (acc is never -0)
                for (unsigned m = 0; m < stride; ++m) {
                    const float2 v = *(x - m);
                    acc.x = acc.x + arm[m] * v.x;
                    acc.y = acc.y + arm[m] * v.y;
                }
                if (!STREAM) {
                    if (t < n_lead) {
                        acc.x = acc.x * s_lead[t];
                        acc.y = acc.y * s_lead[t];
                    } else if (t >= q.n_samples - n_trail) {
                        const float g = s_trail[t - (q.n_samples - n_trail)];
                        acc.x = acc.x * g;
                        acc.y = acc.y * g;
                    }
                }
                r[2 * k + e] = acc;
            }
        }
    }
    const bool wide = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    for (unsigned k = 0; k < kTxPairs; ++k) {
        const unsigned long long s = S0 + 2ull * (k * kTxThreads + threadIdx.x);
        if (s + 1 < S1 && wide) {
            *reinterpret_cast<float4*>(out + s) = make_float4(r[2 * k].x, r[2 * k].y, r[2 * k + 1].x, r[2 * k + 1].y);
        } else {
            if (s < S1) out[s] = r[2 * k];
            if (s + 1 < S1) out[s + 1] = r[2 * k + 1];
        }
    }
}

// stream mode: hist[i] = symbol (total - (stride - 1) + i) of the call, all inside its last packet (>= 212 symbols)
__global__ void k_tx_carry(TxSym a, unsigned last, unsigned stride, float2* __restrict__ hist)
{
    const unsigned i = threadIdx.x;
    if (i + 1 >= stride) return;
    const TxPacket q = a.pk[last];
    hist[i] = tx_symbol(a, q, a.dv[last], tx_symbols(q.len, true) - (stride - 1) + i);
}

} // namespace

struct gr4pm_packet_transmitter {
    unsigned sps = 4, stride = 12;
    bool stream_mode = false;
    size_t max_packets = 0, max_payload_bytes = 0;
    hipStream_t stream = nullptr;
    uint32_t glfsr = 1; // the GLFSR register at the next burst (glfsr_source.hpp:85-89: seed 1)
    float qa = 0.f;
    std::vector<uint32_t> jump; // [32][32]: the columns of M18^(2^k), M18 = 18 GLFSR steps
    DevBuf<uint32_t> d_consts, d_jump;
    DevBuf<float> d_taps;
    DevBuf<uint8_t> d_scr;
    DevBuf<TxPacket> d_pk;
    DevBuf<TxDerived> d_dv;
    DevBuf<unsigned> d_tiles;
    DevBuf<float2> d_hist;
    std::vector<TxPacket> h_pk;
};

namespace {

unsigned long long tx_burst_samples(const gr4pm_packet_transmitter* h, uint64_t len)
{
    const unsigned long long syms = kSyncSymbols + kHeaderSymbols + 4 * (len + 4) +
                                    (h->stream_mode ? 0 : kRampSymbols + kFlushSymbols);
    return syms * h->sps;
}

// the checks of process(): nothing is written before they pass
gr4pm_status tx_plan(const gr4pm_packet_transmitter* h, const uint64_t* lengths, const uint8_t* packet_types,
                     const uint64_t* gaps, size_t n_packets, unsigned long long* n_out, unsigned long long* n_bytes)
{
    if (n_packets > h->max_packets) {
        set_error("%zu packets in one call, max_packets is %zu", n_packets, h->max_packets);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n_packets && !lengths) {
        set_error("null lengths");
        return GR4PM_ERR_INVALID;
    }
    if (gaps && h->stream_mode) {
        for (size_t i = 0; i < n_packets; ++i)
            if (gaps[i]) {
                set_error("gaps are a burst mode setting");
                return GR4PM_ERR_INVALID;
            }
    }
    unsigned long long total = 0, bytes = 0;
    for (size_t i = 0; i < n_packets; ++i) {
        if (lengths[i] == 0) { // packet_ingress.hpp:171-172
            set_error("packet %zu: packet_length = 0", i);
            return GR4PM_ERR_INVALID;
        }
        if (lengths[i] > kMaxPacketLength) { // header_formatter.hpp:102-106
            set_error("packet %zu: packet_length %llu is too large", i, static_cast<unsigned long long>(lengths[i]));
            return GR4PM_ERR_INVALID;
        }
        if (packet_types && packet_types[i] > 1) {
            set_error("packet %zu: packet_type %u is neither USER_DATA (0) nor IDLE (1)", i, packet_types[i]);
            return GR4PM_ERR_INVALID;
        }
        if (gaps && gaps[i] > (1ull << 40)) {
            set_error("packet %zu: gap of %llu samples", i, static_cast<unsigned long long>(gaps[i]));
            return GR4PM_ERR_INVALID;
        }
        bytes += lengths[i];
        total += (gaps ? gaps[i] : 0) + tx_burst_samples(h, lengths[i]);
    }
    if (bytes > h->max_payload_bytes) {
        set_error("%llu payload bytes in one call, max_payload_bytes is %zu", bytes, h->max_payload_bytes);
        return GR4PM_ERR_OVERFLOW;
    }
    *n_out = total;
    *n_bytes = bytes;
    return GR4PM_OK;
}

} // namespace

extern "C" {

gr4pm_status gr4pm_packet_transmitter_create(const gr4pm_packet_transmitter_params* p, gr4pm_packet_transmitter** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    if (p->samples_per_symbol == 0 || p->samples_per_symbol > kTxMaxSps || p->max_packets == 0 ||
        p->max_packets > (1u << 30)) {
        set_error("samples_per_symbol must be in [1, %u] and max_packets in [1, 2^30]", kTxMaxSps);
        return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_packet_transmitter> h(new (std::nothrow) gr4pm_packet_transmitter);
    if (!h) return GR4PM_ERR_NOMEM;
    h->sps = static_cast<unsigned>(p->samples_per_symbol);
    h->stream_mode = p->stream_mode != 0;
    h->max_packets = p->max_packets;
    h->max_payload_bytes = p->max_payload_bytes;
    h->stream = static_cast<hipStream_t>(p->stream);
    h->qa = std::sqrt(2.0f) / 2.0f;
    const unsigned sps = h->sps;

    // packet_transmitter_rrc_taps.hpp:8-28: the RRC scaled so that the largest polyphase |tap| sum is 0.9
    std::vector<float> rrc(sps * 11 + 1);
    const size_t n_rrc = gr4pm_firdes_root_raised_cosine(1.0, static_cast<double>(sps), 1.0, 0.35, sps * 11, rrc.data());
    if (n_rrc == 0) return GR4PM_ERR_NOMEM;
    float worst = 0.0f;
    for (unsigned j = 0; j < sps; ++j) {
        float acc = 0.0f;
        for (size_t k = j; k < n_rrc; k += sps) acc = acc + std::fabs(rrc[k]);
        worst = std::max(worst, acc);
    }
    const float scale = 0.9f / worst;
    h->stride = static_cast<unsigned>((n_rrc + sps - 1) / sps);
    std::vector<float> taps(sps * h->stride + 19 * sps, 0.0f);
    for (size_t k = 0; k < n_rrc; ++k) taps[(k % sps) * h->stride + k / sps] = rrc[k] * scale;
    // packet_transmitter_pdu.hpp:296-313: ramps of offset + ramp = 8 sps and flush - offset + ramp = 11 sps samples
    float* lead = taps.data() + sps * h->stride;
    float* trail = lead + 8 * sps;
    const double half_pi = 0.5 * 3.14159265358979323846;
    for (unsigned j = 0; j < 8 * sps; ++j)
        lead[j] = static_cast<float>(std::sin(static_cast<double>(j + 1) / static_cast<double>(8 * sps) * half_pi));
    for (unsigned j = 0; j < 11 * sps; ++j)
        trail[11 * sps - 1 - j] =
            static_cast<float>(std::sin(static_cast<double>(j + 1) / static_cast<double>(11 * sps) * half_pi));

    std::vector<uint32_t> consts(kConstWords, 0);
    for (uint32_t b = 0; b < 256; ++b) { // Crc<uint32_t>, reflected input (crc.hpp)
        uint32_t c = b;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
        consts[kConstCrc + b] = c;
    }
    consts[kConstX2n] = 1u << 30; // x^1
    for (unsigned k = 1; k < 32; ++k) consts[kConstX2n + k] = multmodp(consts[kConstX2n + k - 1], consts[kConstX2n + k - 1]);
    if (!p->header_generator) {
        set_error("header_generator (96 rows of the LDPC(128,32) generator) is required");
        return GR4PM_ERR_INVALID;
    }
    std::copy(p->header_generator, p->header_generator + 96, consts.begin() + kConstGen);

    h->jump.assign(32 * 32, 0);
    for (unsigned i = 0; i < 32; ++i) {
        uint32_t r = 1u << i;
        for (unsigned s = 0; s < 2 * kRampSymbols; ++s) r = glfsr_step(r);
        h->jump[i] = r;
    }
    for (unsigned k = 1; k < 32; ++k)
        for (unsigned i = 0; i < 32; ++i) h->jump[32 * k + i] = gf2_apply(&h->jump[32 * (k - 1)], h->jump[32 * (k - 1) + i]);

    // AdditiveScrambler(mask 0x4001, seed 0x18E38, length 16), restarted at every packet (:118-122): its output for
    // the longest body, header included
    const size_t scr_bytes = 32 + std::min<size_t>(kMaxPacketLength, std::max<size_t>(p->max_payload_bytes, 1)) + 4;
    std::vector<uint8_t> scr(scr_bytes, 0);
    uint64_t reg = 0x18E38;
    for (size_t i = 0; i < 8 * scr_bytes; ++i) { // additive_scrambler.hpp:84-87
        scr[i >> 3] |= static_cast<uint8_t>((reg & 1) << (7 - (i & 7)));
        reg = (static_cast<uint64_t>(__builtin_parityll(reg & 0x4001)) << 16) | (reg >> 1);
    }

    const size_t tiles = 1; // grown per call
    GR4PM_TRY(h->d_consts.alloc(consts.size()));
    GR4PM_TRY(h->d_consts.upload(consts.data(), consts.size(), h->stream));
    GR4PM_TRY(h->d_jump.alloc(h->jump.size()));
    GR4PM_TRY(h->d_jump.upload(h->jump.data(), h->jump.size(), h->stream));
    GR4PM_TRY(h->d_taps.alloc(taps.size()));
    GR4PM_TRY(h->d_taps.upload(taps.data(), taps.size(), h->stream));
    GR4PM_TRY(h->d_scr.alloc(scr.size()));
    GR4PM_TRY(h->d_scr.upload(scr.data(), scr.size(), h->stream));
    GR4PM_TRY(h->d_pk.alloc(h->max_packets));
    GR4PM_TRY(h->d_pk.reserve_stage(h->max_packets));
    GR4PM_TRY(h->d_dv.alloc(h->max_packets));
    GR4PM_TRY(h->d_tiles.alloc(tiles));
    GR4PM_TRY(h->d_hist.alloc(h->stride));
    GR4PM_TRY(h->d_hist.zero(h->stream));
    return finish_create(h, out, "packet_transmitter");
}
GR4PM_ABI_CATCH

void gr4pm_packet_transmitter_destroy(gr4pm_packet_transmitter* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_packet_transmitter_reset(gr4pm_packet_transmitter* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    h->glfsr = 1;
    GR4PM_TRY(h->d_hist.zero(h->stream));
    GR4PM_HIP_TRY(hipStreamSynchronize(h->stream));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_packet_transmitter_output_items(const gr4pm_packet_transmitter* h, const uint64_t* lengths,
                                                   const uint8_t* packet_types, const uint64_t* gaps, size_t n_packets,
                                                   size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    unsigned long long total = 0, bytes = 0;
    GR4PM_TRY(tx_plan(h, lengths, packet_types, gaps, n_packets, &total, &bytes));
    *n_out = static_cast<size_t>(total);
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_packet_transmitter_process(gr4pm_packet_transmitter* h, const uint8_t* payload,
                                              const uint64_t* lengths, const uint8_t* packet_types,
                                              const uint64_t* gaps, size_t n_packets, gr4pm_c64* out, size_t out_cap,
                                              uint64_t* burst_offsets, uint64_t* burst_lengths, size_t* n_out)
try {
    if (!h || !n_out) return GR4PM_ERR_INVALID;
    unsigned long long total = 0, bytes = 0;
    GR4PM_TRY(tx_plan(h, lengths, packet_types, gaps, n_packets, &total, &bytes));
    if (total > out_cap) {
        set_error("out_cap %zu, the call makes %llu samples", out_cap, total);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n_packets && (!payload || !out || !burst_offsets || !burst_lengths)) {
        set_error("null pointer");
        return GR4PM_ERR_INVALID;
    }
    *n_out = 0;
    if (n_packets == 0) return GR4PM_OK;
    h->h_pk.resize(n_packets);
    unsigned long long pos = 0, in_off = 0;
    for (size_t i = 0; i < n_packets; ++i) {
        TxPacket& q = h->h_pk[i];
        pos += gaps ? gaps[i] : 0;
        q.in_off = in_off;
        q.out_off = pos;
        q.n_samples = static_cast<unsigned>(tx_burst_samples(h, lengths[i]));
        q.len = static_cast<unsigned>(lengths[i]);
        q.type = packet_types ? packet_types[i] : 0;
        q.pad = 0;
        burst_offsets[i] = pos;
        burst_lengths[i] = q.n_samples;
        pos += q.n_samples;
        in_off += lengths[i];
    }
    const unsigned long long tiles = (total + kTxTile - 1) / kTxTile;
    if (h->d_tiles.n < tiles) GR4PM_TRY(h->d_tiles.alloc(tiles + tiles / 4));
    GR4PM_TRY(h->d_pk.upload_staged(h->h_pk.data(), n_packets, h->stream));
    const unsigned n = static_cast<unsigned>(n_packets);
    hipLaunchKernelGGL(k_tx_prepass, dim3((n + kTxThreads / 64 - 1) / (kTxThreads / 64)), dim3(kTxThreads), 0, h->stream,
                       h->d_pk.p, n, payload, h->d_consts.p, h->d_jump.p, h->glfsr, h->d_tiles.p, h->d_dv.p);
    TxSym a{h->d_pk.p, h->d_dv.p, payload, h->d_scr.p, h->qa};
    const size_t smem = tx_smem(h->sps, h->stride);
    float2* o = reinterpret_cast<float2*>(out);
    if (h->stream_mode)
        hipLaunchKernelGGL(k_tx_samples<true>, dim3(static_cast<unsigned>(tiles)), dim3(kTxThreads), smem, h->stream, a, n,
                           h->d_tiles.p, h->d_taps.p, h->sps, h->stride, h->d_hist.p, total, o);
    else
        hipLaunchKernelGGL(k_tx_samples<false>, dim3(static_cast<unsigned>(tiles)), dim3(kTxThreads), smem, h->stream, a, n,
                           h->d_tiles.p, h->d_taps.p, h->sps, h->stride, h->d_hist.p, total, o);
    if (h->stream_mode)
        hipLaunchKernelGGL(k_tx_carry, dim3(1), dim3(64), 0, h->stream, a, n - 1, h->stride, h->d_hist.p);
    GR4PM_HIP_TRY(hipGetLastError());
    h->glfsr = glfsr_jump(h->jump.data(), h->glfsr, h->stream_mode ? 0 : n_packets);
    *n_out = static_cast<size_t>(total);
    // the packet table's staging area is reused by the next call: it waits for this one
    GR4PM_HIP_TRY(hipStreamSynchronize(h->stream));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
