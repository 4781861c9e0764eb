// Host emulation of one segment of k_fft_filter (gr4-packet-modem_amd/csrc/fft_filter.hip) on the one-exchange wave FFT
// (fft2048_w64.hpp): the 64 lanes run phase by phase on the CPU -- forward transform, the product with the table in the
// kernel's layout and with its components swapped (conj(X) W), the same transform again, the swap back -- and the kept
// samples p >= V are compared with the direct convolution in double.  Built and run by tests/test_fft_filter_ref.py (no GPU
// needed); the arithmetic is plain float here, where the kernel uses packed instructions.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <random>
#include <vector>
#include "fft2048_w64.hpp"

using namespace gr4pm;
using cd = std::complex<double>;

static std::vector<f4> tT(kW64TwFloat4);
static std::vector<cf> cc(64);

// the whole transform for all 64 lanes: r[lane][j] = v[lane + 64 j] in, X[lane + 64 j] out
static void fft_w64(std::vector<std::vector<cf>>& r)
{
    std::vector<float> xb(kW64BufDwords, 0.f);
    for (int l = 0; l < 64; ++l) dft32(r[l].data());
    for (int l = 0; l < 64; ++l) w64_store_ref(l, r[l].data(), xb.data());
    for (int l = 0; l < 64; ++l) w64_mid(l, xb.data(), tT.data(), cc[l], r[l].data());
    for (int l = 0; l < 64; ++l) dft32(r[l].data());
}

// a float4 of the table, two bins
struct f4h {
    float x, y, z, w;
};

int main()
{
    build_w64_tables(
        [](int k) {
            const double a = -2.0 * M_PI * k / kFftN;
            return mk(static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a)));
        },
        tT.data(), cc.data());
    std::mt19937 rng(7);
    std::normal_distribution<float> g(0.f, 1.f);
    const int L = 200, V = 256, N = kFftN;
    std::vector<cd> h(L), x(N);
    for (auto& v : h) v = cd(g(rng), g(rng)) / 14.0;
    for (auto& v : x) v = cd(g(rng), g(rng));
    // make_table as fft_filter.hip
    std::vector<f4h> G(16 * 64);
    for (int k = 0; k < N; ++k) {
        cd acc = 0;
        for (int t = 0; t < L; ++t) {
            const double a = -2.0 * M_PI * ((k * t) % N) / N;
            acc += h[t] * cd(std::cos(a), std::sin(a));
        }
        const float gr = (float)(acc.real() / N), gi = (float)(acc.imag() / N);
        const int lane = k % 64, j = k / 64;
        f4h& q = G[(j / 2) * 64 + lane];
        if (j % 2 == 0) q.x = gi, q.y = gr; else q.z = gi, q.w = gr;
    }
    std::vector<std::vector<cf>> r(64, std::vector<cf>(32));
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 32; ++j) r[l][j] = mk((float)x[l + 64 * j].real(), (float)x[l + 64 * j].imag());
    fft_w64(r);
    for (int l = 0; l < 64; ++l)
        for (int u = 0; u < 16; ++u) {
            const f4h q = G[64 * u + l];
            auto cc_ = [](cf a, cf w) { return mk(a.x * w.x + a.y * w.y, a.x * w.y - a.y * w.x); };
            r[l][2 * u] = cc_(r[l][2 * u], mk(q.x, q.y));
            r[l][2 * u + 1] = cc_(r[l][2 * u + 1], mk(q.z, q.w));
        }
    fft_w64(r);
    double e = 0, m = 0;
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 32; ++j) {
            const int p = l + 64 * j;
            if (p < V) continue;
            cd want = 0;
            for (int t = 0; t < L; ++t) want += h[t] * x[p - t];
            const cd got(r[l][j].y, r[l][j].x); // swap_xy
            e = std::max(e, std::abs(got - want));
            m = std::max(m, std::abs(want));
        }
    std::printf("filter emu max_rel_err %.3e\n", e / m);
    return e / m < 1e-5 ? 0 : 1;
}
