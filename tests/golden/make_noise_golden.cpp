// Writes the reference NoiseSource's output stream (raw little-endian floats) to stdout, for
// tests/golden/make_noise_golden.py.  The generator is the reference's own random.hpp, included from the
// reference checkout at build time (nothing of it is committed); the per-sample expressions below are those
// of NoiseSource::processBulk (noise_source.hpp), so the toolchain that compiles this file -- ROCm clang++
// against libstdc++, -std=c++23 -- decides the argument order of std::complex(gasdev(), gasdev()) exactly as
// it does for the reference.
//
//   make_noise_golden <c64|float> <uniform|gaussian|laplacian|impulse> <seed> <amplitude> <n_items>
#include <gnuradio-4.0/packet-modem/random.hpp>

#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numbers>
#include <string>
#include <vector>

using Rng = gr::packet_modem::random;

int main(int argc, char** argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s <c64|float> <type> <seed> <amplitude> <n>\n", argv[0]);
        return 2;
    }
    const std::string item = argv[1], type = argv[2];
    const uint64_t seed = std::strtoull(argv[3], nullptr, 0);
    const float amplitude = std::strtof(argv[4], nullptr);
    const size_t n = std::strtoull(argv[5], nullptr, 0);
    const float amplitude_complex = amplitude / std::numbers::sqrt2_v<float>;
    Rng rng(seed); // NoiseSource::start()
    const size_t chunk = 1 << 16;
    if (item == "c64") {
        std::vector<std::complex<float>> buf(chunk);
        for (size_t done = 0; done < n; done += chunk) {
            const size_t m = std::min(chunk, n - done);
            for (size_t i = 0; i < m; ++i) {
                auto& x = buf[i];
                if (type == "uniform")
                    x = std::complex<float>(amplitude_complex * ((rng.ran1() * 2.0f) - 1.0f),
                                            amplitude_complex * ((rng.ran1() * 2.0f) - 1.0f));
                else if (type == "gaussian")
                    x = amplitude_complex * rng.rayleigh_complex();
                else
                    return 3; // the reference throws "invalid noise_type"
            }
            std::fwrite(buf.data(), sizeof(buf[0]), m, stdout);
        }
    } else if (item == "float") {
        std::vector<float> buf(chunk);
        for (size_t done = 0; done < n; done += chunk) {
            const size_t m = std::min(chunk, n - done);
            for (size_t i = 0; i < m; ++i) {
                auto& x = buf[i];
                if (type == "uniform")
                    x = static_cast<float>(amplitude * ((rng.ran1() * 2.0f) - 1.0f));
                else if (type == "gaussian")
                    x = static_cast<float>(amplitude * rng.gasdev());
                else if (type == "laplacian")
                    x = static_cast<float>(amplitude * rng.laplacian());
                else if (type == "impulse")
                    x = static_cast<float>(amplitude * rng.impulse(9));
                else
                    return 3;
            }
            std::fwrite(buf.data(), sizeof(buf[0]), m, stdout);
        }
    } else {
        return 2;
    }
    return 0;
}
