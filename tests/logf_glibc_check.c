// glibc >= 2.28 logf (sysdeps/ieee754/flt-32/e_logf.c, e_logf_data.c: Szabolcs Nagy's optimized-routines
// table of 16 (1/c, log c) pairs plus a degree-3 polynomial in double, one rounding) restated; exhaustive
// comparison with the host libm for every float in [0, 2] (the arguments the noise source's logf sees).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <pthread.h>
#ifndef FMA
#define FMA 1
#endif
#if FMA
#define MADD(a, b, c) fma((a), (b), (c))
#else
#define MADD(a, b, c) ((a) * (b) + (c))
#endif
static const double INVC[16] = {
    0x1.661ec79f8f3bep+0, 0x1.571ed4aaf883dp+0, 0x1.49539f0f010bp+0, 0x1.3c995b0b80385p+0,
    0x1.30d190c8864a5p+0, 0x1.25e227b0b8eap+0, 0x1.1bb4a4a1a343fp+0, 0x1.12358f08ae5bap+0,
    0x1.0953f419900a7p+0, 0x1p+0, 0x1.e608cfd9a47acp-1, 0x1.ca4b31f026aap-1,
    0x1.b2036576afce6p-1, 0x1.9c2d163a1aa2dp-1, 0x1.886e6037841edp-1, 0x1.767dcf5534862p-1};
static const double LOGC[16] = {
    -0x1.57bf7808caadep-2, -0x1.2bef0a7c06ddbp-2, -0x1.01eae7f513a67p-2, -0x1.b31d8a68224e9p-3,
    -0x1.6574f0ac07758p-3, -0x1.1aa2bc79c81p-3, -0x1.a4e76ce8c0e5ep-4, -0x1.1973c5a611cccp-4,
    -0x1.252f438e10c1ep-5, 0x0p+0, 0x1.aa5aa5df25984p-5, 0x1.c5e53aa362eb4p-4,
    0x1.526e57720db08p-3, 0x1.bc2860d22477p-3, 0x1.1058bc8a07ee1p-2, 0x1.4043057b6ee09p-2};
static const double LN2 = 0x1.62e42fefa39efp-1;
static const double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;

static float my_logf(float x)
{
    uint32_t ix;
    memcpy(&ix, &x, 4);
    if (ix == 0x3f800000u) return 0.0f;
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
        if (ix * 2 == 0) return -INFINITY;
        if (ix == 0x7f800000u) return x;
        if ((ix & 0x80000000u) || ix * 2 >= 0xff000000u) return NAN;
        float xs = x * 0x1p23f; // subnormal: normalize
        memcpy(&ix, &xs, 4);
        ix -= 23u << 23;
    }
    uint32_t tmp = ix - 0x3f330000u;
    int i = (tmp >> 19) % 16;
    int k = (int32_t)tmp >> 23;
    uint32_t iz = ix - (tmp & 0xff800000u);
    float zf;
    memcpy(&zf, &iz, 4);
    double z = zf;
    double r = MADD(z, INVC[i], -1.0);
    double y0 = LOGC[i] + (double)k * LN2;
    double r2 = r * r;
    double y = MADD(A1, r, A2);
    y = MADD(A0, r2, y);
    y = MADD(y, r2, y0 + r);
    return (float)y;
}

enum { T = 16 };
typedef struct { uint32_t lo, hi; long bad; uint32_t first_bad; } job;
static void* run(void* p)
{
    job* j = (job*)p;
    for (uint32_t u = j->lo; u < j->hi; ++u) {
        float x, a, b;
        memcpy(&x, &u, 4);
        a = logf(x);
        b = my_logf(x);
        if (memcmp(&a, &b, 4) != 0) {
            if (!j->bad) j->first_bad = u;
            ++j->bad;
        }
    }
    return 0;
}
int main()
{
    const uint32_t top = 0x40000000u + 1; // [0, 2]: +0 .. 2.0f inclusive
    pthread_t th[T]; job jb[T];
    for (int i = 0; i < T; ++i) {
        jb[i].lo = (uint32_t)((uint64_t)top * i / T); jb[i].hi = (uint32_t)((uint64_t)top * (i + 1) / T);
        jb[i].bad = 0; jb[i].first_bad = 0;
        pthread_create(&th[i], 0, run, &jb[i]);
    }
    long bad = 0;
    for (int i = 0; i < T; ++i) { pthread_join(th[i], 0); bad += jb[i].bad; if (jb[i].bad) printf("first bad 0x%08x\n", jb[i].first_bad); }
    printf("FMA=%d: %u floats in [0, 2]: logf mismatches %ld\n", FMA, top, bad);
    return 0;
}
