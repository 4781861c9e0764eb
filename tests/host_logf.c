// The host libm's logf over a run of consecutive float bit patterns: the target of test_noise_source.py's device sweep.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

void host_logf_range(uint32_t first_bits, size_t n, float* out)
{
    for (size_t i = 0; i < n; ++i) {
        const uint32_t u = first_bits + (uint32_t)i;
        float x;
        memcpy(&x, &u, 4);
        out[i] = logf(x);
    }
}
