// A sequential restatement of the reference NoiseSource's stream (noise_source.hpp, random.hpp, xoroshiro128p.h as
// compiled by ROCm clang++ against libstdc++), written from the semantics alone: the CPU side of
// tests/test_noise_source.py (2^24-item digests) and tests/test_channel_loopback.py (the loopback stimulus).
// Build with -ffp-contract=off: every float operation rounds on its own, as in the reference's x86-64 baseline build.
//
//   noise_ref_stream <c64|float> <uniform|gaussian|laplacian|impulse> <seed> <amplitude> <n_items>
// writes the n items as raw little-endian floats (complex: re, im) to stdout.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t S[2];
static int stored;
static float stored_val;

static inline uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
static inline uint64_t next(void)
{
    const uint64_t s0 = S[0];
    uint64_t s1 = S[1];
    const uint64_t r = s0 + s1;
    s1 ^= s0;
    S[0] = rotl(s0, 55) ^ s1 ^ (s1 << 14);
    S[1] = rotl(s1, 36);
    return r;
}
static void seed(uint64_t v)
{
    // state[0] = seed; state[1] = splitmix64 step (which advances state[0] by its gamma); then the 2^64 jump
    uint64_t z = (S[0] = v + 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    S[1] = z ^ (z >> 31);
    static const uint64_t JUMP[2] = {0xbeac0467eba5facbull, 0xd86b048b86aa9922ull};
    uint64_t a0 = 0, a1 = 0;
    for (int i = 0; i < 2; ++i)
        for (int b = 0; b < 64; ++b) {
            if (JUMP[i] & (1ull << b)) { a0 ^= S[0]; a1 ^= S[1]; }
            next();
        }
    S[0] = a0;
    S[1] = a1;
    stored = 0;
}
// generate_canonical<float, 24>: float(u) rounded to nearest, times 2^-64; 1.0 becomes nextafter(1, 0)
static inline float ran1(void)
{
    float r = (float)next() * 0x1p-64f;
    return r >= 1.0f ? 0x1.fffffep-1f : r;
}
static float gasdev(void)
{
    if (stored) { stored = 0; return stored_val; }
    float x, y, s;
    do {
        x = 2.0f * ran1() - 1.0f;
        y = 2.0f * ran1() - 1.0f;
        s = x * x + y * y;
    } while (s >= 1.0f || s == 0.0f);
    const float f = sqrtf(-2.0f * logf(s) / s);
    stored = 1;
    stored_val = x * f;
    return y * f;
}

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const int c64 = strcmp(argv[1], "c64") == 0;
    const char* t = argv[2];
    const int type = !strcmp(t, "uniform") ? 0 : !strcmp(t, "gaussian") ? 1 : !strcmp(t, "laplacian") ? 2
                     : !strcmp(t, "impulse") ? 3 : -1;
    if (type < 0 || (c64 && type > 1)) return 3;
    seed(strtoull(argv[3], 0, 0));
    const float amp = strtof(argv[4], 0);
    const float amp_c = amp / 1.41421356237309504880f;
    const size_t n = strtoull(argv[5], 0, 0);
    enum { CH = 1 << 16 };
    static float buf[2 * CH];
    for (size_t done = 0; done < n; done += CH) {
        const size_t m = n - done < CH ? n - done : CH;
        for (size_t i = 0; i < m; ++i) {
            if (c64) {
                float re, im;
                if (type == 0) {
                    re = amp_c * ((ran1() * 2.0f) - 1.0f);
                    im = amp_c * ((ran1() * 2.0f) - 1.0f);
                } else {
                    const float g1 = gasdev(); // std::complex(gasdev(), gasdev()), left to right
                    const float g2 = gasdev();
                    re = amp_c * g1;
                    im = amp_c * g2;
                }
                buf[2 * i] = re;
                buf[2 * i + 1] = im;
            } else {
                float v;
                if (type == 0) {
                    v = amp * ((ran1() * 2.0f) - 1.0f);
                } else if (type == 1) {
                    v = amp * gasdev();
                } else if (type == 2) {
                    const float z = ran1();
                    v = amp * (z > 0.5f ? -logf(2.0f * (1.0f - z)) : logf(2.0f * z));
                } else {
                    const float z = -1.41421356237309504880f * logf(ran1());
                    v = amp * (fabsf(z) <= 9.0f ? 0.0f : z);
                }
                buf[i] = v;
            }
        }
        fwrite(buf, sizeof(float) * (c64 ? 2 : 1), m, stdout);
    }
    return 0;
}
