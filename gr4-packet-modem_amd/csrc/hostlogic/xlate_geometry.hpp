// hostlogic/xlate_geometry.hpp -- the tiles of the four kernels of csrc/ddc.hip and csrc/duc.hip: the sizes the
// kernels and their creates share, and per kernel one pure function from the block's shape (I, D, the prototype's
// length L, the channels K) to what the kernel needs that does not change from call to call: a `tile`, the member of
// the kernel's argument struct that the kernel reads, and what the launch takes beside it.  HIP-free:
// tests/hostlogic/xlate_geometry_check.cpp sweeps every shape the creates admit and asserts what the kernels rest on
// (the LDS each takes, the bounds of every index they divide by a reciprocal word).
#pragma once
#include <cstddef>
#include <cstdint>

namespace gr4pm {
namespace hostlogic {

constexpr int kNt = 256;       // threads of a workgroup, and the most frames of a tile
constexpr int kGroup = 8;      // channels of a Ddc workgroup
constexpr unsigned kWave = 64; // lanes of a wave, and the most items per branch of a rational Ddc tile
constexpr size_t kDdcStageItems = 8192;     // complex64 items of LDS of a Ddc workgroup: 64 KiB
constexpr size_t kDucTileItems = 2048;      // output samples of a Duc tile, about
constexpr size_t kDucStageItems = 2048;     // complex64 items of k_duc's stage: 16 KiB
constexpr unsigned kRotBlock = 1024;        // B: the rational Duc rotator's aligned block of absolute output indices
constexpr unsigned kRotSpan = 3;            // aligned blocks that a tile of at most 2048 samples touches
constexpr size_t kRducLdsItems = 6144;      // complex64 items of LDS a rational Duc tile aims at: 48 KiB ...
constexpr size_t kRducLdsItemsMost = 10240; // ... and what it may take where one sample per branch needs more: 80 KiB

// ceil(2^32 / n) for n >= 2: with e = n rcp - 2^32 < n, j rcp / 2^32 = j / n + j e / (n 2^32), whose floor is j div n
// while j e < 2^32.  So j div n = umulhi(j, reciprocal_word(n)) for every j < 2^32 / n: j < 2^22 at n <= 1024.
inline unsigned reciprocal_word(size_t n) { return n >= 2 ? static_cast<unsigned>(((uint64_t(1) << 32) + n - 1) / n) : 0u; }

struct DdcTile {
    unsigned T;    // frames of a tile
    unsigned Lc;   // taps of a chunk
    unsigned RS;   // items of a stage row (odd)
    unsigned rcpD; // reciprocal_word(D): the kernel divides stage indices, below RS D <= 2^13
};
struct DdcGeometry {
    DdcTile tile;
    unsigned smem; // bytes of dynamic LDS
};

inline DdcGeometry ddc_geometry(size_t D, size_t L)
{
    // the tile: rows of `cols` items (made odd), D rows within the stage; a tile of T frames and a chunk of Lc taps
    // use T + (Lc - 1) div D columns.  All of L in one chunk where 256 frames leave room for it, else half the columns
    // go to frames and the rest to taps.
    size_t cols = kDdcStageItems / D;
    if (cols % 2 == 0) --cols; // >= 7
    const size_t extra_all = (L - 1) / D;
    size_t T = kNt, extra = extra_all;
    if (T + extra_all > cols) {
        T = cols / 2 < static_cast<size_t>(kNt) ? cols / 2 : static_cast<size_t>(kNt);
        extra = cols - T < extra_all ? cols - T : extra_all;
    }
    DdcGeometry g;
    g.tile.T = static_cast<unsigned>(T);
    g.tile.Lc = static_cast<unsigned>((extra + 1) * D < L ? (extra + 1) * D : L);
    g.tile.RS = static_cast<unsigned>((T + extra) | 1);
    g.tile.rcpD = reciprocal_word(D);
    g.smem = static_cast<unsigned>(static_cast<size_t>(g.tile.RS) * D * 8);
    return g;
}

struct RddcTile {
    unsigned T;    // items per branch of a tile
    unsigned RS;   // items of a stage row (odd)
    unsigned rcpD; // reciprocal_word(D): stage indices, below 2^13
    unsigned Dinv; // D^-1 mod I
};
struct RddcGeometry {
    RddcTile tile;
    unsigned waves; // of a workgroup
    unsigned smem;
};

// false: no tile fits
inline bool rddc_geometry(size_t I, size_t D, size_t L, size_t K, RddcGeometry& g)
{
    const size_t P = (L + I - 1) / I;
    g.tile.Dinv = 0;
    for (size_t v = 1; v < I; ++v)
        if (v * D % I == 1) g.tile.Dinv = static_cast<unsigned>(v);
    // waves of a workgroup: a wave takes a branch at a time, so the count w of 2 .. 4 with the fewest wave slots
    // ceil(I / w) w, the larger one of equals
    size_t waves = 2;
    for (size_t w = 3; w <= kNt / kWave; ++w)
        if ((I + w - 1) / w * w <= (I + waves - 1) / waves * waves) waves = w;
    g.waves = static_cast<unsigned>(waves);
    // the tile: the most items per branch T <= 64 whose stage (D rows of an odd number of items for the
    // ((I T - 1) D + I - 1) div I + P samples that I T consecutive items reach) and results (I T per channel of a
    // group) fit the 64 KiB
    const size_t G = K < static_cast<size_t>(kGroup) ? K : static_cast<size_t>(kGroup);
    size_t T = kWave, RS = 0;
    for (;; --T) {
        if (T == 0) return false;
        const size_t S = ((I * T - 1) * D + I - 1) / I + P;
        RS = ((S + D - 1) / D) | 1;
        if (RS * D + I * T * G <= kDdcStageItems) break;
    }
    g.tile.T = static_cast<unsigned>(T);
    g.tile.RS = static_cast<unsigned>(RS);
    g.tile.rcpD = reciprocal_word(D);
    g.smem = static_cast<unsigned>((RS * D + I * T * G) * 8);
    return true;
}

struct DucTile {
    unsigned IP;     // phases of the table and rows of the tile: I rounded up to a multiple of R
    unsigned T, TS;  // frames of a tile; items of a tile row (odd)
    unsigned WF;     // waves that share the tile's frames: 1, 2 or 4
    unsigned G;      // channels of a group
    unsigned Pc;     // taps per phase of a chunk (P unless G == 1)
    unsigned ZS;     // items of a stage row: T + Pc - 1
    unsigned rcpI;   // reciprocal_word(I): tile indices, below T I <= 2^11
};
struct DucGeometry {
    DucTile tile;
    unsigned R; // phases of a lane: the kernel's template argument
    unsigned smem;
};

inline DucGeometry duc_geometry(size_t I, size_t L, size_t K)
{
    const size_t P = (L + I - 1) / I;
    // the tile: R phases per lane, T frames (even unless I = 1, so that T I is even) of about kDucTileItems samples in
    // all; the stage: whole channels while T + P - 1 items of each fit, else one channel and chunks of the p loop
    const size_t R = I >= 8 ? 8 : I >= 4 ? 4 : I >= 2 ? 2 : 1;
    const size_t IP = (I + R - 1) / R * R;
    size_t T = kDucTileItems / I & ~size_t(1);
    T = T > static_cast<size_t>(kNt) ? static_cast<size_t>(kNt) : T < 2 ? 2 : T;
    size_t G = 1, Pc = P;
    if (T + P - 1 <= kDucStageItems) {
        G = kDucStageItems / (T + P - 1);
        if (G > K) G = K;
    } else {
        Pc = kDucStageItems - T + 1;
    }
    DucGeometry g;
    g.R = static_cast<unsigned>(R);
    g.tile.IP = static_cast<unsigned>(IP);
    g.tile.T = static_cast<unsigned>(T);
    g.tile.TS = static_cast<unsigned>(T | 1);
    g.tile.WF = T <= 64 ? 1u : T <= 128 ? 2u : 4u;
    g.tile.G = static_cast<unsigned>(G);
    g.tile.Pc = static_cast<unsigned>(Pc);
    g.tile.ZS = static_cast<unsigned>(T + Pc - 1);
    g.tile.rcpI = reciprocal_word(I);
    g.smem = static_cast<unsigned>((IP * g.tile.TS + G * g.tile.ZS) * 8); // at most 29 KiB + 16 KiB
    return g;
}

struct RducTile {
    unsigned T, TS;      // samples per branch of a tile; items of a tile row (odd)
    unsigned chunks;     // ceil(T / 64): a wave takes 64 samples of a branch at a time
    unsigned S, RS;      // items of a row that a tile spans; items of a stage row (odd)
    unsigned G;          // channels of a group
    unsigned rcpI, rcpD; // reciprocal_word(n): the kernel divides indices below I (D + 1), L + I, D + P and S, all < 2^17
};
struct RducGeometry {
    RducTile tile;
    unsigned smem;
};

// false: no tile fits
inline bool rduc_geometry(size_t I, size_t D, size_t L, size_t K, RducGeometry& g)
{
    const size_t P = (L + I - 1) / I;
    // the tile: T samples per branch, about kDucTileItems in all and whole waves of a branch where that gives 64 or
    // more; the stage: D rows of an odd number of items for the ((I T - 1) D + I - 1) div I + P items that I T
    // consecutive samples reach.  The largest T whose tile and one channel's stage fit kRducLdsItems, or T = 1 in
    // kRducLdsItemsMost; then as many channels to a group as fit.  The taps are never chunked.
    size_t T = kDucTileItems / I;
    T = T >= 64 ? (T > static_cast<size_t>(kNt) ? static_cast<size_t>(kNt) : T / 64 * 64) : (T < 1 ? 1 : T);
    size_t S = 0, RS = 0, budget = kRducLdsItems;
    for (;;) {
        S = ((I * T - 1) * D + I - 1) / I + P;
        RS = ((S + D - 1) / D) | 1;
        if (I * (T | 1) + kRotSpan + D * RS <= budget) break;
        if (T == 1) {
            if (budget == kRducLdsItemsMost) return false;
            budget = kRducLdsItemsMost;
        } else {
            T -= T > 64 ? 64 : 1;
        }
    }
    size_t G = (budget - I * (T | 1)) / (D * RS + kRotSpan);
    if (G > K) G = K;
    g.tile.T = static_cast<unsigned>(T);
    g.tile.TS = static_cast<unsigned>(T | 1);
    g.tile.chunks = static_cast<unsigned>((T + 63) / 64);
    g.tile.S = static_cast<unsigned>(S);
    g.tile.RS = static_cast<unsigned>(RS);
    g.tile.G = static_cast<unsigned>(G);
    g.tile.rcpI = reciprocal_word(I);
    g.tile.rcpD = reciprocal_word(D);
    g.smem = static_cast<unsigned>((I * g.tile.TS + G * (D * RS + kRotSpan)) * 8);
    return true;
}

} // namespace hostlogic
} // namespace gr4pm
