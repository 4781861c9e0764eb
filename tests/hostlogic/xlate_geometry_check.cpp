// A stand-alone sweep of csrc/hostlogic/xlate_geometry.hpp (the tiles of k_ddc, k_ddc_rational, k_duc and
// k_duc_rational), built with -fsanitize=undefined,address by tests/test_xlate_geometry.py.  For every shape the
// creates admit -- every D of the Ddc, every I of the Duc, every coprime pair of the rational forms, K = 1 .. 8 and 64,
// L at the edges of every branch of the arithmetic -- it asserts what the kernels rest on: the LDS a tile takes, the
// ranges of its sizes, and that every index a kernel divides by a reciprocal word divides exactly.
// stdout: "refused ddc|duc I D L K" per shape that no tile fits (with the argument "refused": otherwise only their
// count), then one line of counts.  Exit status 1 and a line per failure on stderr where an assertion fails.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "hostlogic/xlate_geometry.hpp"

using namespace gr4pm::hostlogic;

static int g_failures = 0;
static const char* g_kernel = "";
static size_t g_I, g_D, g_L, g_K;

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond) && ++g_failures <= 50)                                                                                   \
            std::fprintf(stderr, "%s I=%zu D=%zu L=%zu K=%zu: %s\n", g_kernel, g_I, g_D, g_L, g_K, #cond);                   \
    } while (0)

static const size_t kKs[] = {1, 2, 3, 4, 5, 6, 7, 8, 64};
static const size_t kMaxL = 8192;

// the prototype lengths at which the arithmetic of a shape turns
static std::vector<size_t> lengths(size_t I, size_t D)
{
    const size_t raw[] = {1, I - 1, I, I + 1, D, D + 1, 12 * std::max(I, D), kMaxL};
    std::vector<size_t> out;
    for (size_t l : raw) {
        l = std::min(std::max(l, size_t(1)), kMaxL);
        if (std::find(out.begin(), out.end(), l) == out.end()) out.push_back(l);
    }
    return out;
}

// the largest index divided by the reciprocal word of n, per kernel
static size_t most_ddc[1025], most_rddc[1025], most_duc[1025], most_rduc_I[1025], most_rduc_D[65];
static void most(size_t* table, size_t n, size_t j) { table[n] = std::max(table[n], j); }

static void check_ddc(size_t D, size_t L)
{
    g_kernel = "k_ddc", g_I = 1, g_D = D, g_L = L, g_K = 0;
    const DdcGeometry geo = ddc_geometry(D, L);
    const DdcTile& g = geo.tile;
    CHECK(geo.smem == g.RS * D * 8 && geo.smem <= kDdcStageItems * 8);
    CHECK(g.T >= 1 && g.T <= 256);
    CHECK(g.Lc >= 1 && g.Lc <= L);
    CHECK(g.RS % 2 == 1 && g.RS > g.T - 1 + (g.Lc - 1) / D);
    CHECK(g.RS * D <= 8192);
    CHECK(g.rcpD == reciprocal_word(D));
    most(most_ddc, D, (g.T - 1) * D + g.Lc - 1); // the stage fill's last j
}

static bool check_rddc(size_t I, size_t D, size_t L, size_t K)
{
    g_kernel = "k_ddc_rational", g_I = I, g_D = D, g_L = L, g_K = K;
    RddcGeometry geo;
    if (!rddc_geometry(I, D, L, K, geo)) return false;
    const RddcTile& g = geo.tile;
    const size_t P = (L + I - 1) / I, G = std::min(K, size_t(8));
    CHECK(geo.smem == (g.RS * D + I * g.T * G) * 8 && geo.smem <= kDdcStageItems * 8);
    CHECK(g.T >= 1 && g.T <= 64);
    const size_t S = ((I * g.T - 1) * D + I - 1) / I + P;
    CHECK(g.RS % 2 == 1 && g.RS * D >= S);
    CHECK(g.RS * D + I * g.T * G <= 8192);
    CHECK(geo.waves >= 2 && geo.waves <= 4);
    CHECK(g.Dinv * D % I == 1);
    CHECK(g.rcpD == reciprocal_word(D));
    most(most_rddc, D, S - 1); // the stage fill's last j
    return true;
}

static void check_duc(size_t I, size_t L, size_t K)
{
    g_kernel = "k_duc", g_I = I, g_D = 1, g_L = L, g_K = K;
    const DucGeometry geo = duc_geometry(I, L, K);
    const DucTile& g = geo.tile;
    const size_t P = (L + I - 1) / I;
    CHECK(geo.smem == (g.IP * g.TS + g.G * g.ZS) * 8 && geo.smem <= 48 * 1024);
    CHECK((geo.R == 1 || geo.R == 2 || geo.R == 4 || geo.R == 8) && geo.R <= I);
    CHECK(g.IP % geo.R == 0 && I <= g.IP && g.IP < I + geo.R);
    CHECK(g.T >= 2 && g.T <= 256 && g.T * I % 2 == 0);
    CHECK(g.TS % 2 == 1 && g.TS >= g.T);
    CHECK(64 * g.WF >= g.T && (g.WF == 1 || g.WF == 2 || g.WF == 4));
    CHECK(g.G >= 1 && g.G <= K);
    CHECK(g.ZS == g.T + g.Pc - 1 && g.G * g.ZS <= 2048);
    CHECK(g.Pc >= 1 && (g.Pc == P || g.G == 1) && g.Pc <= P);
    CHECK(g.rcpI == reciprocal_word(I));
    most(most_duc, I, g.T * I - 1); // the tile store's last j
}

static bool check_rduc(size_t I, size_t D, size_t L, size_t K)
{
    g_kernel = "k_duc_rational", g_I = I, g_D = D, g_L = L, g_K = K;
    RducGeometry geo;
    if (!rduc_geometry(I, D, L, K, geo)) return false;
    const RducTile& g = geo.tile;
    const size_t P = (L + I - 1) / I;
    CHECK(geo.smem == (I * g.TS + g.G * (D * g.RS + kRotSpan)) * 8 && geo.smem <= kRducLdsItemsMost * 8);
    CHECK(g.T >= 1 && I * g.T <= 2048); // what makes kRotSpan enough: (1023 + 2048 - 1) div 1024 + 1 = 3
    CHECK((kRotBlock - 1 + I * g.T - 1) / kRotBlock + 1 <= kRotSpan);
    CHECK(g.chunks == (g.T + 63) / 64);
    CHECK(g.TS % 2 == 1 && g.TS >= g.T);
    CHECK(g.S == ((I * g.T - 1) * D + I - 1) / I + P);
    CHECK(g.RS % 2 == 1 && D * g.RS >= g.S);
    CHECK(g.G >= 1 && g.G <= K);
    CHECK(I * g.TS + g.G * (D * g.RS + kRotSpan) <= 10240);
    CHECK(g.rcpI == reciprocal_word(I) && g.rcpD == reciprocal_word(D));
    // by rcpI: a unit u < I chunks, b0 + q D with b0, q < I, L - r + I - 1 with r >= 0, a tile sample t < I T
    most(most_rduc_I, I, std::max(std::max(I * g.chunks - 1, (I - 1) * (D + 1)), std::max(L + I - 1, I * g.T - 1)));
    // by rcpD: a stage item s < S, and e + P - 1 with e = (b0 + q D) div I <= D
    most(most_rduc_D, D, std::max<size_t>(g.S - 1, D + P - 1));
    return true;
}

static void check_words(const char* kernel, const size_t* table, size_t n_most)
{
    g_kernel = kernel, g_I = g_L = g_K = 0;
    for (size_t n = 2; n <= n_most; ++n) {
        g_D = n;
        const uint64_t rcp = reciprocal_word(n);
        bool exact = table[n] < (uint64_t(1) << 22);
        for (uint64_t j = 0; j <= table[n]; ++j) exact = exact && ((j * rcp) >> 32) == j / n;
        CHECK(exact);
    }
}

int main(int argc, char** argv)
{
    const bool list = argc > 1 && !std::strcmp(argv[1], "refused");
    size_t n_shapes = 0, n_refused = 0;
    for (size_t D = 1; D <= 1024; ++D)
        for (size_t L : lengths(1, D)) check_ddc(D, L), ++n_shapes;
    for (size_t I = 1; I <= 1024; ++I)
        for (size_t L : lengths(I, 1))
            for (size_t K : kKs) check_duc(I, L, K), ++n_shapes;
    // the rational forms: the Ddc's pairs have I in 2 .. 64 (I = 1 is k_ddc's), the Duc's D in 2 .. 64
    for (size_t a = 2; a <= 64; ++a)
        for (size_t b = 1; b <= 1024; ++b) {
            if (std::gcd(a, b) != 1) continue;
            for (size_t K : kKs) {
                for (size_t L : lengths(a, b)) {
                    ++n_shapes;
                    if (!check_rddc(a, b, L, K)) {
                        ++n_refused;
                        if (list) std::printf("refused ddc %zu %zu %zu %zu\n", a, b, L, K);
                    }
                }
                for (size_t L : lengths(b, a)) {
                    ++n_shapes;
                    if (!check_rduc(b, a, L, K)) {
                        ++n_refused;
                        if (list) std::printf("refused duc %zu %zu %zu %zu\n", b, a, L, K);
                    }
                }
            }
        }
    check_words("k_ddc rcpD", most_ddc, 1024);
    check_words("k_ddc_rational rcpD", most_rddc, 1024);
    check_words("k_duc rcpI", most_duc, 1024);
    check_words("k_duc_rational rcpI", most_rduc_I, 1024);
    check_words("k_duc_rational rcpD", most_rduc_D, 64);
    std::printf("xlate_geometry_check: %zu shapes, %zu refused, %d failures\n", n_shapes, n_refused, g_failures);
    return g_failures ? 1 : 0;
}
