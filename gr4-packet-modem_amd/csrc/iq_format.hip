// iq_format.hip -- integer IQ (sc16, sc8, cu8: include/gr4pm_hip.h) to complex64 and back.
// The project's own block (the reference moves complex64 only).  Pure streaming kernels:
//   A wave owns tiles of 64 x 16 bytes of the INTEGER stream (256 sc16 items, 512 8-bit items).  That side moves as
//   one 16-byte access per lane, 1 KiB contiguous per wave instruction; the complex64 side of the same tile is 2 or 4
//   KiB.  With the natural mapping a lane's 4 or 8 items would meet 16 bytes of complex64 at a 32- or 64-byte
//   stride, so the integer words cross the wave through LDS (1 KiB per wave and tile, written as b128 and read as
//   b64 / b32 when unpacking, the other way round when packing): every complex64 instruction is again 64 x 16
//   contiguous bytes.  Only the wave itself reads what it wrote (the LDS executes a wave's accesses in order), so no
//   workgroup barrier is involved.
//   Pointers are aligned to the item only.  The stream that is WRITTEN is peeled to a 16-byte boundary (a head of up
//   to 1 item when unpacking, 3 or 7 when packing) and a tail below one tile follows; both go an item per lane.  The
//   stream that is READ then sits at any multiple of its item: its 16-byte loads need no alignment on this target.
//   Grid: up to 2048 workgroups of four waves (8 waves per SIMD on 256 CUs), tiles handed out grid-stride.
// pack counts clipped components per lane, sums them in the wave and the workgroup, and adds the workgroup's total
// with one atomic.
#include "iq_format.hpp"

namespace {

using namespace gr4pm::iq;

constexpr int kNt = 256, kWaves = kNt / 64;
constexpr unsigned kMaxGrid = 2048;
constexpr int kUnpackTiles = 2; // tiles a wave has in flight: 2 x 16 bytes of loads per lane

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// between a wave's LDS writes and its reads of other lanes' words: the hardware keeps the order, the compiler must too
__device__ __forceinline__ void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int F>
__device__ __forceinline__ void store_item(void* p, size_t i, uint32_t w)
{
    if constexpr (Fmt<F>::item_bytes == 4)
        static_cast<uint32_t*>(p)[i] = w;
    else
        static_cast<uint16_t*>(p)[i] = static_cast<uint16_t>(w);
}

template <int F>
__global__ __launch_bounds__(kNt) void k_iq_unpack(const unsigned char* in, size_t in_stride, float scale, size_t rows,
                                                   size_t n, float2* out, size_t out_stride)
{
    constexpr int I = Fmt<F>::item_bytes, IPL = 16 / I, TILE = 64 * IPL, NS = IPL / 2, U = kUnpackTiles;
    __shared__ uint32_t s_x[kWaves][U][256];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (size_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const unsigned char* inr = in + row * in_stride * I;
        float2* outr = out + row * out_stride;
        const size_t misaligned = (reinterpret_cast<uintptr_t>(outr) >> 3) & 1;
        const size_t head = misaligned < n ? misaligned : n;
        const size_t nt = (n - head) / TILE;
        const unsigned char* inb = inr + head * I;
        float2* outb = outr + head; // 16-byte aligned
        for (size_t t0 = (static_cast<size_t>(blockIdx.x) * kWaves + wave) * U; t0 < nt;
             t0 += static_cast<size_t>(gridDim.x) * kWaves * U) {
            u32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (t0 + u < nt) __builtin_memcpy(&v[u], inb + ((t0 + u) * 64 + lane) * 16, 16);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (t0 + u < nt) *reinterpret_cast<u32x4*>(&s_x[wave][u][lane * 4]) = v[u];
            wave_lds_order();
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (t0 + u >= nt) continue;
                float4* o = reinterpret_cast<float4*>(outb + (t0 + u) * TILE);
#pragma unroll
                for (int j = 0; j < NS; ++j) { // items j 128 + 2 lane and the next
                    float2 a, b;
                    if constexpr (I == 4) {
                        const u32x2 r = *reinterpret_cast<const u32x2*>(&s_x[wave][u][(j * 64 + lane) * 2]);
                        a = unpack_item<F>(r.x, scale), b = unpack_item<F>(r.y, scale);
                    } else {
                        const uint32_t r = s_x[wave][u][j * 64 + lane];
                        a = unpack_item<F>(r & 0xFFFFu, scale), b = unpack_item<F>(r >> 16, scale);
                    }
                    o[j * 64 + lane] = float4{a.x, a.y, b.x, b.y};
                }
            }
            wave_lds_order(); // the reads, before the next tiles' writes
        }
        if (blockIdx.x == 0) { // the head and the tail
            const size_t done = head + nt * TILE, rest = head + (n - done);
            for (size_t i = threadIdx.x; i < rest; i += kNt) {
                const size_t idx = i < head ? i : done + (i - head);
                outr[idx] = unpack_item<F>(load_item<F>(inr, idx), scale);
            }
        }
    }
}

template <int F>
__global__ __launch_bounds__(kNt) void k_iq_pack(const float2* in, size_t in_stride, size_t rows, size_t n, float gain,
                                                 unsigned char* out, size_t out_stride, unsigned long long* clipped)
{
    constexpr int I = Fmt<F>::item_bytes, IPL = 16 / I, TILE = 64 * IPL, NL = IPL / 2;
    __shared__ uint32_t s_x[kWaves][256];
    __shared__ unsigned s_clip[kWaves];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned clip = 0;
    for (size_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const float2* inr = in + row * in_stride;
        unsigned char* outr = out + row * out_stride * I;
        const size_t misaligned = ((16 - (reinterpret_cast<uintptr_t>(outr) & 15)) & 15) / I;
        const size_t head = misaligned < n ? misaligned : n;
        const size_t nt = (n - head) / TILE;
        const float2* inb = inr + head;
        unsigned char* outb = outr + head * I; // 16-byte aligned
        for (size_t t = static_cast<size_t>(blockIdx.x) * kWaves + wave; t < nt; t += static_cast<size_t>(gridDim.x) * kWaves) {
            float4 v[NL];
#pragma unroll
            for (int j = 0; j < NL; ++j) // items j 128 + 2 lane and the next: 8-byte aligned
                __builtin_memcpy(&v[j], __builtin_assume_aligned(inb + t * TILE + (j * 64 + lane) * 2, 8), 16);
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const uint32_t w0 = pack_item<F>(float2{v[j].x, v[j].y}, gain, clip);
                const uint32_t w1 = pack_item<F>(float2{v[j].z, v[j].w}, gain, clip);
                if constexpr (I == 4)
                    *reinterpret_cast<u32x2*>(&s_x[wave][(j * 64 + lane) * 2]) = u32x2{w0, w1};
                else
                    s_x[wave][j * 64 + lane] = w0 | (w1 << 16);
            }
            wave_lds_order();
            const u32x4 o = *reinterpret_cast<const u32x4*>(&s_x[wave][lane * 4]);
            reinterpret_cast<u32x4*>(outb + t * 1024)[lane] = o;
            wave_lds_order();
        }
        if (blockIdx.x == 0) {
            const size_t done = head + nt * TILE, rest = head + (n - done);
            for (size_t i = threadIdx.x; i < rest; i += kNt) {
                const size_t idx = i < head ? i : done + (i - head);
                store_item<F>(outr, idx, pack_item<F>(inr[idx], gain, clip));
            }
        }
    }
    if (!clipped) return; // (the same in every thread)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) clip += __shfl_down(clip, d, 64);
    if (lane == 0) s_clip[wave] = clip;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) total += s_clip[w];
        if (total) atomicAdd(clipped, static_cast<unsigned long long>(total));
    }
}

// up to kMaxGrid workgroups in all: as many along a row as it has work for, the rest over the rows
dim3 grid_for(size_t rows, size_t n, size_t tile, size_t tiles_per_wg)
{
    const size_t wgs = (n / tile + tiles_per_wg - 1) / tiles_per_wg;
    const size_t gx = wgs < 1 ? 1 : (wgs > kMaxGrid ? kMaxGrid : wgs);
    size_t gy = kMaxGrid / gx;
    gy = gy < 1 ? 1 : (gy > rows ? rows : gy);
    return dim3(static_cast<unsigned>(gx), static_cast<unsigned>(gy));
}

gr4pm_status check_args(const char* what, const void* in, size_t in_stride, int format, size_t rows, size_t n, const void* out,
                        size_t out_stride)
{
    using gr4pm::set_error;
    if (!valid(format)) {
        set_error("%s: format %d is none of GR4PM_IQ_SC16 / SC8 / CU8", what, format);
        return GR4PM_ERR_INVALID;
    }
    if (rows == 0 || n == 0) return GR4PM_OK;
    if (!in || !out) {
        set_error("%s: a null pointer for %zu items", what, n);
        return GR4PM_ERR_INVALID;
    }
    if (in_stride < n || out_stride < n) {
        set_error("%s: strides of %zu and %zu items for rows of %zu", what, in_stride, out_stride, n);
        return GR4PM_ERR_INVALID;
    }
    return GR4PM_OK;
}

} // namespace

extern "C" {

gr4pm_status gr4pm_iq_unpack(const void* in, size_t in_stride, int format, float scale, size_t rows, size_t n, gr4pm_c64* out,
                             size_t out_stride, void* stream)
try {
    GR4PM_TRY(check_args("iq_unpack", in, in_stride, format, rows, n, out, out_stride));
    if (rows == 0 || n == 0) return GR4PM_OK;
    if (scale == 0.0f) scale = default_scale(format);
    const auto* src = static_cast<const unsigned char*>(in);
    auto* dst = reinterpret_cast<float2*>(out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid = grid_for(rows, n, 1024 / item_bytes(format), kWaves * kUnpackTiles);
    if (format == GR4PM_IQ_SC16)
        hipLaunchKernelGGL(k_iq_unpack<GR4PM_IQ_SC16>, grid, dim3(kNt), 0, s, src, in_stride, scale, rows, n, dst, out_stride);
    else if (format == GR4PM_IQ_SC8)
        hipLaunchKernelGGL(k_iq_unpack<GR4PM_IQ_SC8>, grid, dim3(kNt), 0, s, src, in_stride, scale, rows, n, dst, out_stride);
    else
        hipLaunchKernelGGL(k_iq_unpack<GR4PM_IQ_CU8>, grid, dim3(kNt), 0, s, src, in_stride, scale, rows, n, dst, out_stride);
    GR4PM_HIP_TRY(hipGetLastError());
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_iq_pack(const gr4pm_c64* in, size_t in_stride, size_t rows, size_t n, int format, float gain, void* out,
                           size_t out_stride, unsigned long long* clipped, void* stream)
try {
    GR4PM_TRY(check_args("iq_pack", in, in_stride, format, rows, n, out, out_stride));
    if (rows == 0 || n == 0) return GR4PM_OK;
    if (gain == 0.0f) gain = default_gain(format);
    const auto* src = reinterpret_cast<const float2*>(in);
    auto* dst = static_cast<unsigned char*>(out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid = grid_for(rows, n, 1024 / item_bytes(format), kWaves);
    if (format == GR4PM_IQ_SC16)
        hipLaunchKernelGGL(k_iq_pack<GR4PM_IQ_SC16>, grid, dim3(kNt), 0, s, src, in_stride, rows, n, gain, dst, out_stride, clipped);
    else if (format == GR4PM_IQ_SC8)
        hipLaunchKernelGGL(k_iq_pack<GR4PM_IQ_SC8>, grid, dim3(kNt), 0, s, src, in_stride, rows, n, gain, dst, out_stride, clipped);
    else
        hipLaunchKernelGGL(k_iq_pack<GR4PM_IQ_CU8>, grid, dim3(kNt), 0, s, src, in_stride, rows, n, gain, dst, out_stride, clipped);
    GR4PM_HIP_TRY(hipGetLastError());
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
