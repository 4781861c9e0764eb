// noise_source.hip -- NoiseSource<T> (noise_source.hpp:45-110, random.hpp:95-220, xoroshiro128p.h:39-96) on the
// device, bit-exact with the reference's sequential stream for any call size and any chain of calls.
//
// The stream is xoroshiro128+ behind libstdc++'s generate_canonical<float, 24> (one 64-bit draw per ran1()).  An
// "attempt" is the draws one output step consumes: two for every complex type and for the float Gaussian (the
// Marsaglia polar pair x, y), one for the float uniform / Laplacian / impulse types.  Only the Gaussian attempts can
// be rejected.  Decomposition:
//   k_noise_jump   one wave per tile of TPB * C attempts: the tile's start state, from the seeded state, by the
//                  128 x 128 GF(2) matrices M^(2^k) (built at create) for the set bits of the draw distance.
//   k_noise_count  (Gaussian) each thread jumps from its tile's state to its chunk of C attempts by the polynomial
//                  x^(D C t) mod charpoly(M) (at most 127 steps of the generator), stores that state, counts accepts.
//   k_noise_scan   (Gaussian) exclusive scan of the per-tile accept counts (one workgroup).
//   k_noise_gauss  (Gaussian) workgroup scan of the per-thread counts, then each thread reruns its chunk and puts
//                  each accepted attempt's output at its rank into the tile's LDS stage; the tile's run of items
//                  then leaves in coalesced stores.
//   k_noise_direct (other types) every attempt is an output item: jump, then write.
// The stream position lives on the device (NoisePos: the attempt after the last one used, and the float Gaussian's
// stored half), double-buffered so that the call that reads one copy writes the other; process() never waits.
#include "common.hpp"

#include <cmath>

namespace {

using u64 = unsigned long long;

constexpr int kTpb = 256;         // threads per tile
constexpr int kChunkGauss = 32;   // attempts per thread, Gaussian (count + write pass)
constexpr int kChunkDirect = 128; // attempts per thread, other types
constexpr int kJumpBits = 64;     // M^(2^k), k < 64: draw distances below 2^64

struct NoisePos {
    u64 attempt;      // the next attempt of the stream
    unsigned stored;  // float Gaussian: a half is kept for the next call (random.hpp gasdev)
    float stored_val; // its value, before the amplitude
};

struct State {
    u64 s0, s1;
};

__host__ __device__ __forceinline__ u64 rotl64(u64 x, int k) { return (x << k) | (x >> (64 - k)); }

// xoroshiro128p_next without the output
__host__ __device__ __forceinline__ void step(State& s)
{
    const u64 s1 = s.s1 ^ s.s0;
    s.s0 = rotl64(s.s0, 55) ^ s1 ^ (s1 << 14);
    s.s1 = rotl64(s1, 36);
}

__host__ __device__ __forceinline__ u64 next(State& s)
{
    const u64 r = s.s0 + s.s1;
    step(s);
    return r;
}

// ran1(): generate_canonical<float, 24> over the 64-bit draw (libstdc++: one draw, float(u) * 2^-64, a result of
// 1.0 replaced by nextafter(1, 0)).  The u64 -> float rounding is done in integers, to nearest even, so that it does
// not depend on how the compiler lowers the conversion; the scale by 2^-64 is exact and folded into the exponent.
__device__ __forceinline__ float ran1(u64 u)
{
    if (u == 0) return 0.0f;
    const int lz = __clzll(u);
    const u64 m = u << lz;                       // leading one at bit 63
    unsigned mant = static_cast<unsigned>(m >> 40); // 24 bits
    const u64 rest = m & ((1ull << 40) - 1);
    const unsigned up = (rest > (1ull << 39)) | ((rest == (1ull << 39)) & (mant & 1u));
    mant += up;
    int e = 63 - lz - 64; // exponent of the scaled value
    if (mant == (1u << 24)) { mant >>= 1; ++e; }
    if (e >= 0) return 0x1.fffffep-1f; // float(u) rounded to 2^64: the clamp
    return __uint_as_float((static_cast<unsigned>(e + 127) << 23) | (mant & 0x7fffffu));
}

// glibc >= 2.28 logf (sysdeps/ieee754/flt-32/e_logf.c, e_logf_data.c): 16 (1/c, log c) pairs and a degree-3
// polynomial in double, one rounding to float.  Pinned against the host libm for every float in [0, 2]
// (tests/logf_glibc_check.c, with and without FMA contraction) and on the device by test_noise_source.py.
__constant__ double kLogfInvc[16] = {
    0x1.661ec79f8f3bep+0, 0x1.571ed4aaf883dp+0, 0x1.49539f0f010bp+0, 0x1.3c995b0b80385p+0,
    0x1.30d190c8864a5p+0, 0x1.25e227b0b8eap+0, 0x1.1bb4a4a1a343fp+0, 0x1.12358f08ae5bap+0,
    0x1.0953f419900a7p+0, 0x1p+0, 0x1.e608cfd9a47acp-1, 0x1.ca4b31f026aap-1,
    0x1.b2036576afce6p-1, 0x1.9c2d163a1aa2dp-1, 0x1.886e6037841edp-1, 0x1.767dcf5534862p-1};
__constant__ double kLogfLogc[16] = {
    -0x1.57bf7808caadep-2, -0x1.2bef0a7c06ddbp-2, -0x1.01eae7f513a67p-2, -0x1.b31d8a68224e9p-3,
    -0x1.6574f0ac07758p-3, -0x1.1aa2bc79c81p-3, -0x1.a4e76ce8c0e5ep-4, -0x1.1973c5a611cccp-4,
    -0x1.252f438e10c1ep-5, 0x0p+0, 0x1.aa5aa5df25984p-5, 0x1.c5e53aa362eb4p-4,
    0x1.526e57720db08p-3, 0x1.bc2860d22477p-3, 0x1.1058bc8a07ee1p-2, 0x1.4043057b6ee09p-2};

__device__ __forceinline__ float logf_glibc(float x)
{
    const double Ln2 = 0x1.62e42fefa39efp-1;
    const double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
    unsigned ix = __float_as_uint(x);
    if (ix == 0x3f800000u) return 0.0f;
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
        if (ix * 2 == 0) return -__builtin_huge_valf();
        if (ix == 0x7f800000u) return x;
        if ((ix & 0x80000000u) || ix * 2 >= 0xff000000u) return __builtin_nanf("");
        ix = __float_as_uint(x * 0x1p23f) - (23u << 23); // subnormal: normalize
    }
    const unsigned tmp = ix - 0x3f330000u;
    const int i = (tmp >> 19) & 15;
    const int k = static_cast<int>(tmp) >> 23;
    const unsigned iz = ix - (tmp & 0xff800000u);
    const double z = static_cast<double>(__uint_as_float(iz));
    const double r = __builtin_fma(z, kLogfInvc[i], -1.0);
    const double y0 = kLogfLogc[i] + static_cast<double>(k) * Ln2;
    const double r2 = r * r;
    double y = __builtin_fma(A1, r, A2);
    y = __builtin_fma(A0, r2, y);
    y = __builtin_fma(y, r2, y0 + r);
    return static_cast<float>(y);
}

// one polar attempt (random.hpp gasdev): x = 2 ran1 - 1, y = 2 ran1 - 1, s = x x + y y, rejected for s >= 1 or
// s == 0; f = sqrtf(-2 logf(s) / s).  Every operation rounds on its own (EXACT_FLAGS: no contraction); division and
// square root correctly rounded (div_rn, sqrt_rn).
struct Polar {
    float x, y, s;
    bool ok;
};
__device__ __forceinline__ Polar polar(State& st)
{
    Polar p;
    p.x = 2.0f * ran1(next(st)) - 1.0f;
    p.y = 2.0f * ran1(next(st)) - 1.0f;
    p.s = p.x * p.x + p.y * p.y;
    p.ok = !(p.s >= 1.0f || p.s == 0.0f);
    return p;
}
// Correctly rounded division and square root, whatever the compiler makes of '/' and sqrtf: HIP's __fsqrt_rn, for one,
// is the approximate native square root unless OCML_BASIC_ROUNDED_OPERATIONS is defined, and it put one Gaussian
// sample in seven an ulp off.  The hardware result q is moved to the float whose rounding interval holds the exact
// value, decided in double where every product below is exact: a midpoint of two adjacent floats has 25 significant
// bits, so m * b (b: 24 bits) and m * m fit in 53, and neither can equal a 24-bit a or x (no ties).
// Positive, finite, normal operands and results only (what polar_factor passes).
__device__ __forceinline__ float next_up(float q) { return __uint_as_float(__float_as_uint(q) + 1u); }
__device__ __forceinline__ float next_down(float q) { return __uint_as_float(__float_as_uint(q) - 1u); }
__device__ __forceinline__ float div_rn(float a, float b)
{
    float q = a / b;
    const double da = a, db = b;
    for (int i = 0; i < 3; ++i) {
        const float u = next_up(q), d = next_down(q);
        const double hi = 0.5 * (static_cast<double>(q) + static_cast<double>(u));
        const double lo = 0.5 * (static_cast<double>(q) + static_cast<double>(d));
        q = hi * db < da ? u : (lo * db > da ? d : q);
    }
    return q;
}
__device__ __forceinline__ float sqrt_rn(float x)
{
    float q = __builtin_sqrtf(x);
    const double dx = x;
    for (int i = 0; i < 3; ++i) {
        const float u = next_up(q), d = next_down(q);
        const double hi = 0.5 * (static_cast<double>(q) + static_cast<double>(u));
        const double lo = 0.5 * (static_cast<double>(q) + static_cast<double>(d));
        q = hi * hi < dx ? u : (lo * lo > dx ? d : q);
    }
    return q;
}
// s in (0, 1): -2 logf(s) > 0, and the quotient is a normal float
__device__ __forceinline__ float polar_factor(float s) { return sqrt_rn(div_rn(-2.0f * logf_glibc(s), s)); }

// M^(D C t) applied as a polynomial in M: acc = sum of p_b M^b s (Cayley-Hamilton, p = x^(D C t) mod charpoly)
__device__ __forceinline__ State poly_jump(State s, u64 p0, u64 p1)
{
    State acc = {0, 0};
    const int top = p1 ? 127 - __clzll(p1) : (p0 ? 63 - __clzll(p0) : -1);
    for (int b = 0; b <= top; ++b) {
        const u64 bit = b < 64 ? (p0 >> b) & 1 : (p1 >> (b - 64)) & 1;
        const u64 mask = 0ull - bit;
        acc.s0 ^= s.s0 & mask;
        acc.s1 ^= s.s1 & mask;
        step(s);
    }
    return acc;
}

struct Ctx {
    const u64* jump;   // kJumpBits matrices x 128 columns x 2 words: column j of M^(2^k) = its image of bit j
    const u64* poly;   // kTpb x 2 words: x^(D C t) mod charpoly
    const NoisePos* pos_in;
    NoisePos* pos_out;
    State seeded;      // random(seed): after xoroshiro128p_seed
    int draws;         // D: draws per attempt
    int chunk;         // C: attempts per thread
};

// one wave per tile: the tile's start state, M^(D (A + g T C)) applied to the seeded state, 64 lanes x 2 columns
// per matrix and a butterfly XOR across the wave
__global__ __launch_bounds__(256) void k_noise_jump(Ctx c, unsigned n_tiles, State* tile_state)
{
    const unsigned lane = threadIdx.x & 63;
    const unsigned tile = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (tile >= n_tiles) return;
    const u64 attempt = c.pos_in->attempt + static_cast<u64>(tile) * kTpb * c.chunk;
    u64 d = attempt * static_cast<u64>(c.draws);
    State v = c.seeded;
    while (d) {
        const int k = __ffsll(static_cast<long long>(d)) - 1;
        d &= d - 1;
        const u64* col = c.jump + (static_cast<size_t>(k) * 128 + 2 * lane) * 2;
        const u64 w = lane < 32 ? v.s0 : v.s1;
        const unsigned sh = (2 * lane) & 63;
        const u64 m0 = 0ull - ((w >> sh) & 1), m1 = 0ull - ((w >> (sh + 1)) & 1);
        u64 a0 = (col[0] & m0) ^ (col[2] & m1);
        u64 a1 = (col[1] & m0) ^ (col[3] & m1);
        for (int o = 32; o >= 1; o >>= 1) {
            a0 ^= __shfl_xor(a0, o, 64);
            a1 ^= __shfl_xor(a1, o, 64);
        }
        v.s0 = a0;
        v.s1 = a1;
    }
    if (lane == 0) tile_state[tile] = v;
}

__global__ __launch_bounds__(kTpb) void k_noise_count(Ctx c, const State* tile_state, State* thread_state,
                                                      unsigned* counts, unsigned* tile_counts)
{
    __shared__ unsigned wsum[kTpb / 64];
    const unsigned t = threadIdx.x, g = blockIdx.x;
    State st = poly_jump(tile_state[g], c.poly[2 * t], c.poly[2 * t + 1]);
    const size_t gt = static_cast<size_t>(g) * kTpb + t;
    thread_state[gt] = st;
    unsigned cnt = 0;
    for (int j = 0; j < kChunkGauss; ++j) cnt += polar(st).ok ? 1u : 0u;
    counts[gt] = cnt;
    unsigned w = cnt;
    for (int o = 32; o >= 1; o >>= 1) w += __shfl_xor(w, o, 64);
    if ((t & 63) == 0) wsum[t / 64] = w;
    __syncthreads();
    if (t == 0) {
        unsigned s = 0;
        for (int i = 0; i < kTpb / 64; ++i) s += wsum[i];
        tile_counts[g] = s;
    }
}

// exclusive scan of the tile counts, in place (one workgroup of 1024)
__global__ __launch_bounds__(1024) void k_noise_scan(unsigned* tile_counts, unsigned n_tiles)
{
    __shared__ unsigned part[1024 / 64];
    __shared__ unsigned carry_s;
    const unsigned t = threadIdx.x, lane = t & 63, wv = t / 64;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (unsigned base = 0; base < n_tiles; base += 1024) {
        const unsigned i = base + t;
        const unsigned v = i < n_tiles ? tile_counts[i] : 0u;
        unsigned incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_up(incl, o, 64);
            if (static_cast<int>(lane) >= o) incl += u;
        }
        if (lane == 63) part[wv] = incl;
        __syncthreads();
        unsigned before = carry_s;
        for (unsigned k = 0; k < wv; ++k) before += part[k];
        if (i < n_tiles) tile_counts[i] = before + incl - v;
        __syncthreads();
        if (t == 1023) carry_s = before + incl;
        __syncthreads();
    }
}

// exclusive prefix of v over the workgroup (kTpb threads)
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* part)
{
    const unsigned t = threadIdx.x, lane = t & 63, wv = t / 64;
    unsigned incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(incl, o, 64);
        if (static_cast<int>(lane) >= o) incl += u;
    }
    if (lane == 63) part[wv] = incl;
    __syncthreads();
    unsigned before = 0;
    for (unsigned k = 0; k < wv; ++k) before += part[k];
    return before + incl - v;
}

// Gaussian, write pass.  IS_C64: sample r = amp_c * (y f, x f) of the r-th accepted attempt (clang evaluates the
// two gasdev() calls of std::complex(gasdev(), gasdev()) left to right).  float: the halves y f, x f of accepted
// attempt r are items h + 2 r and h + 2 r + 1, h = 1 when the previous call left a stored half.
// A tile's accepted attempts are ranks [base, base + total), so its output is one contiguous run of items: every
// thread puts its samples into the tile's stage in LDS at their rank, then the workgroup copies the run out (adding
// the signal in the fused form) with consecutive lanes on consecutive items -- one wave instruction moves 512
// contiguous bytes, not 64 scattered 8-byte pieces.  The stage holds the tile's largest possible run (every attempt
// accepted): 64 KiB.
template <bool IS_C64, bool ADD>
__global__ __launch_bounds__(kTpb) void k_noise_gauss(Ctx c, const State* thread_state, const unsigned* counts,
                                                      const unsigned* tile_prefix, float amp, const void* add_in,
                                                      void* out, u64 n)
{
    constexpr int kStage = kTpb * kChunkGauss; // accepted attempts of a tile, at most
    __shared__ float2 stage[kStage];
    unsigned* part = reinterpret_cast<unsigned*>(stage); // the scan's per-wave sums, before the stage is filled
    const unsigned t = threadIdx.x, g = blockIdx.x;
    const size_t gt = static_cast<size_t>(g) * kTpb + t;
    const unsigned cnt = counts[gt];
    const unsigned excl = block_exclusive_scan(cnt, part);
    unsigned total = 0;
    for (int k = 0; k < kTpb / 64; ++k) total += part[k];
    __syncthreads(); // part is read by all before the stage overwrites it
    const u64 base = tile_prefix[g];
    const u64 rank0 = base + excl;
    const NoisePos pin = *c.pos_in;
    const u64 h = IS_C64 ? 0 : (pin.stored ? 1 : 0);
    const u64 m = n - h;                            // items that come from new attempts
    const u64 need = IS_C64 ? n : (m + 1) / 2;      // accepted attempts used
    if (!IS_C64 && gt == 0) {
        float* o = static_cast<float*>(out);
        if (h) {
            const float v = amp * pin.stored_val;
            o[0] = ADD ? static_cast<const float*>(add_in)[0] + v : v;
        }
        if (need == 0) {
            NoisePos p = {pin.attempt, 0u, 0.0f};
            *c.pos_out = p;
        }
    }
    if (rank0 < need) {
        State st = thread_state[gt];
        u64 r = rank0;
        const u64 attempt0 = pin.attempt + gt * kChunkGauss;
        for (int j = 0; j < kChunkGauss && r < need; ++j) {
            const Polar p = polar(st);
            if (!p.ok) continue;
            const float f = polar_factor(p.s);
            const float g1 = p.y * f, g2 = p.x * f;
            const unsigned local = static_cast<unsigned>(r - base); // < total <= kStage
            stage[local] = float2{amp * g1, amp * g2};
            if (r == need - 1) {
                if constexpr (IS_C64) {
                    NoisePos q = {attempt0 + j + 1, 0u, 0.0f};
                    *c.pos_out = q;
                } else {
                    const bool second = h + 2 * r + 1 < n;
                    NoisePos q = {attempt0 + j + 1, second ? 0u : 1u, second ? 0.0f : g2};
                    *c.pos_out = q;
                }
            }
            ++r;
        }
    }
    __syncthreads();
    if constexpr (IS_C64) {
        if (base >= n) return;
        const unsigned run = static_cast<unsigned>(n - base < total ? n - base : total);
        float2* o = static_cast<float2*>(out) + base;
        const float2* a = static_cast<const float2*>(add_in) + base;
        for (unsigned i = t; i < run; i += kTpb) {
            float2 v = stage[i];
            if constexpr (ADD) {
                const float2 s = a[i];
                v.x = s.x + v.x;
                v.y = s.y + v.y;
            }
            o[i] = v;
        }
    } else {
        const u64 first = h + 2 * base; // item of the stage's first half
        if (first >= n) return;
        const unsigned run = static_cast<unsigned>(n - first < 2ull * total ? n - first : 2ull * total);
        const float* sf = reinterpret_cast<const float*>(stage);
        float* o = static_cast<float*>(out) + first;
        const float* a = static_cast<const float*>(add_in) + first;
        for (unsigned i = t; i < run; i += kTpb) {
            const float v = sf[i];
            o[i] = ADD ? a[i] + v : v;
        }
    }
}

// every attempt is one item: TYPE 0 uniform, 2 Laplacian, 3 impulse (float), 0 uniform (c64: two draws)
template <bool IS_C64, int TYPE, bool ADD>
__global__ __launch_bounds__(kTpb) void k_noise_direct(Ctx c, const State* tile_state, float amp, const void* add_in,
                                                       void* out, u64 n)
{
    const unsigned t = threadIdx.x, g = blockIdx.x;
    const u64 first = (static_cast<u64>(g) * kTpb + t) * kChunkDirect;
    const u64 a_pos = c.pos_in->attempt;
    if (first >= n) return;
    State st = poly_jump(tile_state[g], c.poly[2 * t], c.poly[2 * t + 1]);
    const u64 end = first + kChunkDirect < n ? first + kChunkDirect : n;
    for (u64 i = first; i < end; ++i) {
        if constexpr (IS_C64) {
            const float re = amp * ((ran1(next(st)) * 2.0f) - 1.0f);
            const float im = amp * ((ran1(next(st)) * 2.0f) - 1.0f);
            float2 v = {re, im};
            if constexpr (ADD) {
                const float2 a = static_cast<const float2*>(add_in)[i];
                v.x = a.x + v.x;
                v.y = a.y + v.y;
            }
            static_cast<float2*>(out)[i] = v;
        } else {
            const float z = ran1(next(st));
            float v;
            if constexpr (TYPE == GR4PM_NOISE_UNIFORM) {
                v = (z * 2.0f) - 1.0f;
            } else if constexpr (TYPE == GR4PM_NOISE_LAPLACIAN) {
                v = z > 0.5f ? -logf_glibc(2.0f * (1.0f - z)) : logf_glibc(2.0f * z);
            } else {
                const float e = -1.41421356237309504880f * logf_glibc(z);
                v = fabsf(e) <= 9.0f ? 0.0f : e;
            }
            v = amp * v;
            if constexpr (ADD) v = static_cast<const float*>(add_in)[i] + v;
            static_cast<float*>(out)[i] = v;
        }
    }
    if (end == n) {
        NoisePos q = {a_pos + n, 0u, 0.0f};
        *c.pos_out = q;
    }
}

__global__ void k_logf(const float* x, size_t n, float* out)
{
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) out[i] = logf_glibc(x[i]);
}

// ---- host side: the seeded state, the jump matrices and the jump polynomials ----

using u128 = unsigned __int128;

State seeded_state(u64 seed)
{
    // xoroshiro128p_seed: state[0] = seed, state[1] = splitmix64_next(state) -- which advances state[0] by the
    // golden gamma -- then the 2^64 jump
    State s;
    u64 sm = seed + 0x9e3779b97f4a7c15ull;
    u64 z = sm;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    s.s0 = sm;
    s.s1 = z ^ (z >> 31);
    const u64 JUMP[2] = {0xbeac0467eba5facbull, 0xd86b048b86aa9922ull};
    State acc = {0, 0};
    for (int i = 0; i < 2; ++i)
        for (int b = 0; b < 64; ++b) {
            if (JUMP[i] & (1ull << b)) {
                acc.s0 ^= s.s0;
                acc.s1 ^= s.s1;
            }
            step(s);
        }
    return acc;
}

// column j of a 128 x 128 GF(2) matrix as a 128-bit word (bits 0-63: state[0], 64-127: state[1])
using Mat = std::vector<u128>;
inline u128 st2w(const State& s) { return static_cast<u128>(s.s0) | (static_cast<u128>(s.s1) << 64); }
inline State w2st(u128 w) { return State{static_cast<u64>(w), static_cast<u64>(w >> 64)}; }
inline u128 mat_apply(const Mat& m, u128 v)
{
    u128 r = 0;
    for (int j = 0; j < 128; ++j)
        if ((v >> j) & 1) r ^= m[j];
    return r;
}

// minimal polynomial of the generator (Berlekamp-Massey on bit 0 of the state), returned without its x^128 term;
// false unless it has degree 128 (then it is the characteristic polynomial)
bool charpoly(u128* low)
{
    State s = {0x0123456789abcdefull, 0xfedcba9876543210ull};
    const int N = 512;
    std::vector<int> seq(N);
    for (int i = 0; i < N; ++i) {
        seq[i] = static_cast<int>(s.s0 & 1);
        step(s);
    }
    std::vector<int> C(N + 1, 0), B(N + 1, 0), T;
    C[0] = B[0] = 1;
    int L = 0, m = 1;
    for (int n = 0; n < N; ++n) {
        int d = seq[n];
        for (int i = 1; i <= L; ++i) d ^= C[i] & seq[n - i];
        if (!d) {
            ++m;
        } else if (2 * L <= n) {
            T = C;
            for (int i = 0; i + m <= N; ++i) C[i + m] ^= B[i];
            L = n + 1 - L;
            B = T;
            m = 1;
        } else {
            for (int i = 0; i + m <= N; ++i) C[i + m] ^= B[i];
            ++m;
        }
    }
    if (L != 128) return false;
    // connection polynomial C(x) = 1 + c1 x + ... + c128 x^128; characteristic P(x) = x^128 + c1 x^127 + ... + c128
    u128 p = 0;
    for (int i = 1; i <= 128; ++i)
        if (C[i]) p |= static_cast<u128>(1) << (128 - i);
    *low = p;
    return true;
}

inline u128 mulx(u128 a, u128 plow) { return (a >> 127) ? ((a << 1) ^ plow) : (a << 1); }
inline u128 mulmod(u128 a, u128 b, u128 plow)
{
    u128 r = 0;
    for (int i = 127; i >= 0; --i) {
        r = mulx(r, plow);
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}

} // namespace

struct gr4pm_noise_source {
    int item = 0, type = 0;
    float amplitude = 1.0f;
    u64 seed = 0;
    size_t max_items = 0;
    int draws = 1, chunk = kChunkDirect;
    size_t max_tiles = 0;
    hipStream_t stream = nullptr;
    State seeded = {0, 0};
    int cur = 0; // which NoisePos copy holds the position
    gr4pm::DevBuf<u64> d_jump, d_poly;
    gr4pm::DevBuf<NoisePos> d_pos;
    gr4pm::DevBuf<State> d_tile_state, d_thread_state;
    gr4pm::DevBuf<unsigned> d_counts, d_tile_counts;

    bool gaussian() const { return type == GR4PM_NOISE_GAUSSIAN; }
    // accepted attempts a call of n items may use, and the attempts it runs to get them with margin: the accept rate
    // is pi / 4; the margin of 16 sqrt(R) + 64 attempts is over 25 standard deviations of the accept count
    static size_t gauss_attempts(size_t accepted)
    {
        const double r = static_cast<double>(accepted);
        return static_cast<size_t>(std::ceil((r + 16.0 * std::sqrt(r) + 64.0) * 1.2733));
    }
    size_t attempts_for(size_t n) const
    {
        if (!gaussian()) return n;
        return gauss_attempts(item == GR4PM_NOISE_C64 ? n : (n + 1) / 2);
    }
};

using namespace gr4pm;

extern "C" {

gr4pm_status gr4pm_noise_source_create(const gr4pm_noise_source_params* p, gr4pm_noise_source** out)
try {
    if (!p || !out) return GR4PM_ERR_INVALID;
    *out = nullptr;
    if (p->item_kind != GR4PM_NOISE_C64 && p->item_kind != GR4PM_NOISE_FLOAT) {
        set_error("noise source: item_kind must be GR4PM_NOISE_C64 or GR4PM_NOISE_FLOAT");
        return GR4PM_ERR_INVALID;
    }
    if (p->noise_type < GR4PM_NOISE_UNIFORM || p->noise_type > GR4PM_NOISE_IMPULSE) {
        set_error("noise source: unknown noise_type %d", p->noise_type);
        return GR4PM_ERR_INVALID;
    }
    if (p->item_kind == GR4PM_NOISE_C64 && p->noise_type != GR4PM_NOISE_UNIFORM && p->noise_type != GR4PM_NOISE_GAUSSIAN) {
        set_error("noise source: complex items take UNIFORM or GAUSSIAN noise only (noise_source.hpp: invalid noise_type)");
        return GR4PM_ERR_INVALID;
    }
    if (p->max_items == 0 || p->max_items > (size_t(1) << 31)) {
        set_error("noise source: max_items must be in [1, 2^31]");
        return GR4PM_ERR_INVALID;
    }
    GR4PM_TRY(require_device());
    std::unique_ptr<gr4pm_noise_source> h(new (std::nothrow) gr4pm_noise_source);
    if (!h) return GR4PM_ERR_NOMEM;
    h->item = p->item_kind;
    h->type = p->noise_type;
    h->amplitude = p->amplitude;
    h->seed = p->seed;
    h->max_items = p->max_items;
    h->stream = static_cast<hipStream_t>(p->stream);
    h->draws = (p->item_kind == GR4PM_NOISE_C64 || p->noise_type == GR4PM_NOISE_GAUSSIAN) ? 2 : 1;
    h->chunk = h->gaussian() ? kChunkGauss : kChunkDirect;
    h->seeded = seeded_state(p->seed);
    const size_t tile_attempts = static_cast<size_t>(kTpb) * h->chunk;
    h->max_tiles = (h->attempts_for(p->max_items) + tile_attempts - 1) / tile_attempts;

    // M: one step of the generator; M^(2^k) by squaring
    Mat m(128);
    for (int j = 0; j < 128; ++j) {
        State e = w2st(static_cast<u128>(1) << j);
        step(e);
        m[j] = st2w(e);
    }
    std::vector<u64> jump(static_cast<size_t>(kJumpBits) * 128 * 2);
    for (int k = 0; k < kJumpBits; ++k) {
        for (int j = 0; j < 128; ++j) {
            jump[(static_cast<size_t>(k) * 128 + j) * 2] = static_cast<u64>(m[j]);
            jump[(static_cast<size_t>(k) * 128 + j) * 2 + 1] = static_cast<u64>(m[j] >> 64);
        }
        Mat sq(128);
        for (int j = 0; j < 128; ++j) sq[j] = mat_apply(m, m[j]);
        m.swap(sq);
    }
    // x^(D C t) mod charpoly for the threads of a tile
    u128 plow;
    if (!charpoly(&plow)) {
        set_error("noise source: the generator's minimal polynomial is not of degree 128");
        return GR4PM_ERR_INTERNAL;
    }
    u128 xs = 1;
    for (int i = 0; i < h->draws * h->chunk; ++i) xs = mulx(xs, plow);
    std::vector<u64> poly(static_cast<size_t>(kTpb) * 2);
    u128 pt = 1;
    for (int t = 0; t < kTpb; ++t) {
        poly[2 * t] = static_cast<u64>(pt);
        poly[2 * t + 1] = static_cast<u64>(pt >> 64);
        pt = mulmod(pt, xs, plow);
    }
    // self-check of both jump forms against plain stepping
    {
        State a = h->seeded;
        for (int i = 0; i < 3 * h->draws * h->chunk; ++i) step(a);
        u128 via_poly = 0;
        State s = h->seeded;
        const u128 p3 = static_cast<u128>(poly[6]) | (static_cast<u128>(poly[7]) << 64);
        for (int b = 0; b < 128; ++b) {
            if ((p3 >> b) & 1) via_poly ^= st2w(s);
            step(s);
        }
        u128 via_mat = st2w(h->seeded);
        const u64 d = static_cast<u64>(3) * h->draws * h->chunk;
        for (int k = 0; k < 64; ++k)
            if ((d >> k) & 1) {
                Mat mk(128);
                for (int j = 0; j < 128; ++j)
                    mk[j] = static_cast<u128>(jump[(static_cast<size_t>(k) * 128 + j) * 2]) |
                            (static_cast<u128>(jump[(static_cast<size_t>(k) * 128 + j) * 2 + 1]) << 64);
                via_mat = mat_apply(mk, via_mat);
            }
        if (via_poly != st2w(a) || via_mat != st2w(a)) {
            set_error("noise source: jump self-check failed");
            return GR4PM_ERR_INTERNAL;
        }
    }
    GR4PM_TRY(h->d_jump.alloc(jump.size()));
    GR4PM_TRY(h->d_poly.alloc(poly.size()));
    GR4PM_TRY(h->d_pos.alloc(2));
    GR4PM_TRY(h->d_tile_state.alloc(h->max_tiles));
    if (h->gaussian()) {
        const size_t nt = h->max_tiles * kTpb;
        GR4PM_TRY(h->d_thread_state.alloc(nt));
        GR4PM_TRY(h->d_counts.alloc(nt));
        GR4PM_TRY(h->d_tile_counts.alloc(h->max_tiles));
    }
    GR4PM_TRY(h->d_jump.upload(jump.data(), jump.size(), h->stream));
    GR4PM_TRY(h->d_poly.upload(poly.data(), poly.size(), h->stream));
    GR4PM_TRY(h->d_pos.zero(h->stream));
    return finish_create(h, out, "noise source");
}
GR4PM_ABI_CATCH

void gr4pm_noise_source_destroy(gr4pm_noise_source* h)
try {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}
GR4PM_ABI_CATCH_VOID

gr4pm_status gr4pm_noise_source_reset(gr4pm_noise_source* h)
try {
    if (!h) return GR4PM_ERR_INVALID;
    GR4PM_HIP_TRY(hipMemsetAsync(h->d_pos.p + h->cur, 0, sizeof(NoisePos), h->stream));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_noise_source_set_amplitude(gr4pm_noise_source* h, float amplitude)
try {
    if (!h) return GR4PM_ERR_INVALID;
    h->amplitude = amplitude;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_noise_source_process(gr4pm_noise_source* h, const void* add_in, void* out, size_t n)
try {
    if (!h) return GR4PM_ERR_INVALID;
    if (n > h->max_items) {
        set_error("noise source: %zu items, the handle was made for %zu", n, h->max_items);
        return GR4PM_ERR_OVERFLOW;
    }
    if (n == 0) return GR4PM_OK;
    if (!out) return GR4PM_ERR_INVALID;
    const size_t tile_attempts = static_cast<size_t>(kTpb) * h->chunk;
    const unsigned tiles = static_cast<unsigned>((h->attempts_for(n) + tile_attempts - 1) / tile_attempts);
    Ctx c;
    c.jump = h->d_jump.p;
    c.poly = h->d_poly.p;
    c.pos_in = h->d_pos.p + h->cur;
    c.pos_out = h->d_pos.p + (1 - h->cur);
    c.seeded = h->seeded;
    c.draws = h->draws;
    c.chunk = h->chunk;
    const bool c64 = h->item == GR4PM_NOISE_C64;
    // NoiseSource<complex>: _amplitude_complex = amplitude / sqrt2_v<float>
    const float amp = c64 ? h->amplitude / 1.41421356237309504880f : h->amplitude;
    const bool add = add_in != nullptr;
    hipLaunchKernelGGL(k_noise_jump, dim3((tiles + 3) / 4), dim3(256), 0, h->stream, c, tiles, h->d_tile_state.p);
    if (h->gaussian()) {
        hipLaunchKernelGGL(k_noise_count, dim3(tiles), dim3(kTpb), 0, h->stream, c, h->d_tile_state.p,
                           h->d_thread_state.p, h->d_counts.p, h->d_tile_counts.p);
        hipLaunchKernelGGL(k_noise_scan, dim3(1), dim3(1024), 0, h->stream, h->d_tile_counts.p, tiles);
        auto* kern = c64 ? (add ? k_noise_gauss<true, true> : k_noise_gauss<true, false>)
                         : (add ? k_noise_gauss<false, true> : k_noise_gauss<false, false>);
        hipLaunchKernelGGL(kern, dim3(tiles), dim3(kTpb), 0, h->stream, c, h->d_thread_state.p, h->d_counts.p,
                           h->d_tile_counts.p, amp, add_in, out, static_cast<u64>(n));
    } else {
        void (*kern)(Ctx, const State*, float, const void*, void*, u64) = nullptr;
        if (c64) kern = add ? k_noise_direct<true, GR4PM_NOISE_UNIFORM, true> : k_noise_direct<true, GR4PM_NOISE_UNIFORM, false>;
        else if (h->type == GR4PM_NOISE_UNIFORM)
            kern = add ? k_noise_direct<false, GR4PM_NOISE_UNIFORM, true> : k_noise_direct<false, GR4PM_NOISE_UNIFORM, false>;
        else if (h->type == GR4PM_NOISE_LAPLACIAN)
            kern = add ? k_noise_direct<false, GR4PM_NOISE_LAPLACIAN, true> : k_noise_direct<false, GR4PM_NOISE_LAPLACIAN, false>;
        else
            kern = add ? k_noise_direct<false, GR4PM_NOISE_IMPULSE, true> : k_noise_direct<false, GR4PM_NOISE_IMPULSE, false>;
        hipLaunchKernelGGL(kern, dim3(tiles), dim3(kTpb), 0, h->stream, c, h->d_tile_state.p, amp, add_in, out,
                           static_cast<u64>(n));
    }
    GR4PM_HIP_TRY(hipGetLastError());
    h->cur = 1 - h->cur;
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

gr4pm_status gr4pm_logf(const float* x, size_t n, float* out)
try {
    if (!x || !out) return GR4PM_ERR_INVALID;
    GR4PM_TRY(require_device());
    if (n == 0) return GR4PM_OK;
    hipLaunchKernelGGL(k_logf, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, x, n, out);
    GR4PM_HIP_TRY(hipGetLastError());
    GR4PM_HIP_TRY(hipStreamSynchronize(nullptr));
    return GR4PM_OK;
}
GR4PM_ABI_CATCH

} // extern "C"
