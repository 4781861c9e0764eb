// stream_blocks.hpp -- what more than one of the stream-block units needs (rotator.hip, costas_loop.hip, stream_blocks.hip,
// fir_resamplers.hip, packet_control_blocks.hip): complex arithmetic, the FIR family's item helpers and history kernel,
// table upload, grid sizing, the timing-experiment switch.  The reference headers cited at the entry points are relative
// to the reference's blocks/include/gnuradio-4.0/packet-modem/.
// The units are compiled with -ffp-contract=off: the reference evaluates every product and sum separately (baseline
// x86-64, std::inner_product / std::complex), and the FIR outputs here are bit-exact with that order.
// Pattern shared by all blocks: tags are sparse, so the tag-driven control flow of the
// reference (which is per-chunk C++ on the CPU) is replayed on the host over the TAG LIST
// only -- never over samples -- and turned into a small table of segments/runs; the kernels
// then process every sample / symbol of the call in parallel from that table.  That replay is
// HIP-free code under hostlogic/ (built and checked on the CPU by tests/hostlogic/): the units
// keep the device side -- buffers, uploads, streams and events, kernel choice, launches.  Recurrences
// whose float rounding makes them order dependent (rotator phasor, Costas PLL, resampler
// phase accumulator) run serially per independent segment (one lane each).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "common.hpp"
#include "hostlogic/base.hpp"

namespace gr4pm {
#ifndef GR4PM_SERIAL_PRIO
#define GR4PM_SERIAL_PRIO 3 // s_setprio of the Costas kernels (A/B: make EXTRA=-DGR4PM_SERIAL_PRIO=0)
#endif
#ifndef GR4PM_ROT_PRIO
#define GR4PM_ROT_PRIO GR4PM_SERIAL_PRIO // ... of k_rot_checkpoints, the one serial kernel that runs BESIDE correlator waves
#endif
// GR4PM_TIMING_SKIP=name[,name]: timing experiments only -- the named kernels are not launched (their outputs are
// garbage); tells what a kernel costs the pipelined chain, which its duration alone does not
#ifndef GR4PM_EXPERIMENTS
static constexpr bool timing_skip(const char*) { return false; } // the shipped library leaves no kernel out
#else
static inline bool timing_skip(const char* name)
{
    // comma-separated list, whole names ("symf" does not match "symf_fake"); read once, announced on stderr
    static const char* e = gr4pm::experiment_env("GR4PM_TIMING_SKIP", true);
    if (!e) return false;
    const size_t n = strlen(name);
    for (const char* p = e; (p = strstr(p, name)) != nullptr; p += n)
        if ((p == e || p[-1] == ',') && (p[n] == 0 || p[n] == ',')) return true;
    return false;
}
#endif
namespace { // internal linkage: the library has one code object per unit, each with its own copy

using hostlogic::cf; // hostlogic/base.hpp: the tables the host planners fill hold it
__host__ __device__ __forceinline__ cf cmul(cf a, cf b)
{
    return { a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x };
}
__host__ __device__ __forceinline__ cf cadd(cf a, cf b) { return { a.x + b.x, a.y + b.y }; }
__host__ __device__ __forceinline__ cf fmulc(float t, cf z) { return { t * z.x, t * z.y }; }

// std::abs(std::complex<float>) == hypotf; glibc evaluates it as
// (float)sqrt((double)x*x + (double)y*y), reproduced here with IEEE double ops.
__device__ __forceinline__ float hypot_like_glibc(float x, float y)
{
    const double dx = x, dy = y;
    return static_cast<float>(sqrt(dx * dx + dy * dy));
}

inline size_t bit_ceil_sz(size_t v)
{
    size_t c = 1;
    while (c < v) c <<= 1;
    return c;
}

// =====================================================================================
// FIR family.  x(i) for i < 0 comes from the carried history (last `cap` items of the
// previous calls, zero at start: the reference pre-fills its HistoryBuffer with zeros).
// =====================================================================================
template <typename T>
__device__ __forceinline__ T item_at(const T* cur, const T* carry, unsigned cap, long long i)
{
    return i >= 0 ? cur[i] : carry[static_cast<long long>(cap) + i];
}
__device__ __forceinline__ cf mac(cf acc, float t, cf x) { return cadd(acc, fmulc(t, x)); }
__device__ __forceinline__ float mac(float acc, float t, float x) { return acc + t * x; }
__device__ __forceinline__ cf scale_item(float s, cf v) { return fmulc(s, v); }
__device__ __forceinline__ float scale_item(float s, float v) { return s * v; }
__device__ __forceinline__ cf zero_item(cf) { return { 0.f, 0.f }; }
__device__ __forceinline__ float zero_item(float) { return 0.f; }

template <typename T>
__global__ void k_update_hist(const T* __restrict__ in, const T* __restrict__ carry,
                              T* __restrict__ carry_next, unsigned cap, size_t n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    carry_next[i] = item_at(in, carry, cap, static_cast<long long>(n) - cap + i);
}

constexpr size_t kFirMaxSmem = 160 * 1024; // LDS a workgroup of the FIR family may ask for

template <typename T>
gr4pm_status upload_vec(DevBuf<T>& buf, const std::vector<T>& v, hipStream_t s)
{
    if (buf.n < v.size()) GR4PM_TRY(buf.alloc(std::max<size_t>(v.size() * 2, 64)));
    return buf.upload_staged(v.data(), v.size(), s);
}

inline unsigned grid_for(size_t n, unsigned block, unsigned cap = 65535u * 16u)
{
    const size_t g = (n + block - 1) / block;
    return static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>(g, cap)));
}

} // namespace
} // namespace gr4pm
