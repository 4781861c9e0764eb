#include <mutex>
#include <sys/mman.h>
#include <unistd.h>
#include <thread>
#include <atomic>
// Drives the GR4 block wrappers (gr4-packet-modem_amd/host/gr4pm_gr4_blocks.hpp) through processBulk()
// the way the gnuradio4 scheduler would, against the test-only API stand-in tests/gr4_stub/.
//
// The blocks are reached exactly as a reference flowgraph reaches them: by the reference's header names
// (the include path puts gr4-packet-modem_amd/host first) and with the reference's spellings --
// SyncwordDetection, SyncwordDetectionFilter<>, CoarseFrequencyCorrection<>, SymbolFilter<c64, c64, float>,
// SyncwordWipeoff<>, CostasLoop<> in namespace gr::packet_modem -- wired and parameterised like
// PacketReceiver (packet_receiver.hpp:34-127).  A miniature single-threaded scheduler cuts the chunks at
// tag positions (a tag is only ever seen at the head of a chunk: coarse_frequency_correction.hpp:76-82).
//
// usage: gr4_blocks_driver chain <in.c64> <out_prefix> <host_output 0|1> <max_chunk> <packet_length>
//        gr4_blocks_driver receiver ... (same arguments): the front end, then PacketReceiver's wiring behind it
//            (packet_receiver.hpp:123-139,208-240): PayloadMetadataInsert<> -> CostasLoop<> (steered by its tags) ->
//            SyncwordRemove<> -> ConstellationLLRDecoder<> -> AdditiveScrambler<float> -> HeaderPayloadSplit<> ->
//            HeaderFecDecoder, and the symbol split of zmq_output (:159-162) HeaderPayloadSplit<c64>; writes
//            .llr.f32 / .hdr_llr.f32 / .pay_llr.f32 / .hdr_bytes.u8 / .hdr_sym.c64 / .pay_sym.c64 / .tail_counts.bin
//        gr4_blocks_driver blocks <in.c64> <out_prefix>      (Rotator, InterpolatingFirFilter, PfbArbResampler)
//        gr4_blocks_driver floats <in.f32> <out_prefix>      (test/qa_symbol_filter.cpp:17-63: InterpolatingFirFilter<float,
//            float, float> -> SymbolFilter<float, float, float>; writes .fir.f32 / .sym.f32)
//        gr4_blocks_driver zmq <n_pdus>                      (ZmqPduPubSink<c64> on an ephemeral port, printed first; waits
//            for a subscriber, then publishes n_pdus PDUs through processOne(): PDU k holds 128 (k % 3 == 0) or 100 + 37 k
//            symbols (k, i))
//        gr4_blocks_driver pdus <bits.u8> <symbols.c64> <out_prefix>   (the PDU forms of packet_transmitter_pdu.hpp:119,288:
//            AdditiveScrambler<Pdu<uint8_t>> and InterpolatingFirFilter<Pdu<c64>, Pdu<c64>, float> through processOne()
//            on PDUs of ragged sizes; writes .scr.u8 / .fir.c64 / .scr_sizes.u64 / .fir_sizes.u64 / .fir_tag_index.u64)
// writes <out_prefix>.sd.c64 / .sd_tags.bin / .symbols.c64 / .sym_tags.bin (tests/test_gr4_blocks.py reads them)
#include <gnuradio-4.0/packet-modem/coarse_frequency_correction.hpp>
#include <gnuradio-4.0/packet-modem/costas_loop.hpp>
#include <gnuradio-4.0/packet-modem/firdes.hpp>
#include <gnuradio-4.0/packet-modem/interpolating_fir_filter.hpp>
#include <gnuradio-4.0/packet-modem/pfb_arb_resampler.hpp>
#include <gnuradio-4.0/packet-modem/rotator.hpp>
#include <gnuradio-4.0/packet-modem/symbol_filter.hpp>
#include <gnuradio-4.0/packet-modem/syncword_detection.hpp>
#include <gnuradio-4.0/packet-modem/syncword_detection_filter.hpp>
#include <gnuradio-4.0/packet-modem/syncword_wipeoff.hpp>
// the blocks behind the front end (packet_receiver.hpp:123-139,159-162), `receiver` mode
#include <gnuradio-4.0/packet-modem/additive_scrambler.hpp>
#include <gnuradio-4.0/packet-modem/constellation_llr_decoder.hpp>
#include <gnuradio-4.0/packet-modem/header_fec_decoder.hpp>
#include <gnuradio-4.0/packet-modem/header_payload_split.hpp>
#include <gnuradio-4.0/packet-modem/payload_metadata_insert.hpp>
#include <gnuradio-4.0/packet-modem/syncword_remove.hpp>
// the sink of the symbol tap (packet_receiver.hpp:163-168), `zmq` mode
#include <gnuradio-4.0/packet-modem/zmq_pdu_pub_sink.hpp>
#if !__has_include(<gnuradio-4.0/packet-modem/pdu.hpp>)
namespace gr::packet_modem { // pdu.hpp:15-21 by shape (the reference's header is not on this include path)
template <typename T>
struct Pdu {
    using value_type = T;
    std::vector<T> data{};
    std::vector<gr::Tag> tags{};
};
} // namespace gr::packet_modem
#endif

#include "gr4_mini_scheduler.hpp"

using namespace gr::packet_modem;

// two outputs (HeaderPayloadSplit): one processBulk() with the chunk cut at the next tag; the block publishes its tags
// on the ports `header` / `payload` (header_payload_split.hpp:83-87)
template <typename Blk, typename T>
static bool step_split(Blk& blk, Edge<T>& in, Edge<T>& hdr, Edge<T>& pay, size_t max_chunk)
{
    const size_t start = in.rd;
    if (start >= in.size) return false;
    const size_t end = std::min({ in.size, start + max_chunk, in.next_tag_after(start) });
    blk._mergedInputTag = {};
    if (const gr::Tag* t = in.tag_at(start)) blk._mergedInputTag = { 0, t->map };
    const size_t n = std::min({ end - start, hdr.data.size() - hdr.size, pay.data.size() - pay.size });
    if (n == 0) return false;
    gr::InSpan<T> is(in.data.data() + start, n);
    gr::OutSpan<T> hs(hdr.data.data() + hdr.size, n), ps(pay.data.data() + pay.size, n);
    blk.header.published_tags.clear();
    blk.payload.published_tags.clear();
    const auto st = blk.processBulk(is, hs, ps);
    if (!is.consume_called || !hs.publish_called || !ps.publish_called) throw std::runtime_error("HeaderPayloadSplit: consume / publish missing");
    for (const auto& t : blk.header.published_tags) hdr.tags.push_back({ static_cast<ssize_t>(hdr.size) + t.index, t.map });
    for (const auto& t : blk.payload.published_tags) pay.tags.push_back({ static_cast<ssize_t>(pay.size) + t.index, t.map });
    in.rd += is.consumed;
    hdr.size += hs.published;
    pay.size += ps.published;
    return st == gr::work::Status::OK && is.consumed != 0;
}

static int chain(int argc, char** argv, bool tail = false)
{
    if (argc < 7) return 2;
    const auto x = read_c64(argv[2]);
    const std::string prefix = argv[3];
    const bool host_output = std::atoi(argv[4]) != 0;
    const size_t max_chunk = static_cast<size_t>(std::atoll(argv[5]));
    const uint64_t packet_length = static_cast<uint64_t>(std::atoll(argv[6]));
    const size_t sps = 4;

    // ---- the constants of PacketReceiver's constructor (packet_receiver.hpp:45-122)
    const std::vector<uint8_t> syncword = { 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1,
                                            1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0,
                                            1, 0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0 };
    auto rrc = firdes::root_raised_cosine(1.0, static_cast<double>(sps), 1.0, 0.35, sps * 11);
    float norm = 0.0f;
    for (float t : rrc) norm += t * t;
    norm = std::sqrt(norm);
    for (auto& t : rrc) t /= norm;

    // every block is created and configured as PacketReceiver's constructor does it: fg.emplaceBlock<T>(property_map)
    // with the literal keys and value expressions of packet_receiver.hpp:76-127 (benchmark_syncword_detection.cpp:64-70
    // uses the same six keys for the detector).  The stand-in's Graph assigns the settings BY NAME through the member
    // lists the wrappers register with ENABLE_REFLECTION, and throws for a key a block does not have.
    gr::stub::Graph fg;
    const auto& rrc_taps = rrc;
    const size_t samples_per_symbol = sps;
    const int syncword_freq_bins = 4;
    const float syncword_threshold = 9.5f;
    const std::vector<c64> bpsk_constellation = { { 1.0f, 0.0f }, { -1.0f, 0.0f } };
    auto& syncword_detection = fg.emplaceBlock<SyncwordDetection>({ { "rrc_taps", rrc_taps },
                                                                     { "syncword", syncword },
                                                                     { "constellation", bpsk_constellation },
                                                                     { "min_freq_bin", -syncword_freq_bins },
                                                                     { "max_freq_bin", syncword_freq_bins },
                                                                     { "power_threshold", syncword_threshold } });
    auto& syncword_filter = fg.emplaceBlock<SyncwordDetectionFilter<>>({ { "samples_per_symbol", samples_per_symbol } });
    auto& freq_correction =
        fg.emplaceBlock<CoarseFrequencyCorrection<>>({ { "delay", (rrc_taps.size() - 1) / 2 + samples_per_symbol } });
    const size_t symbol_filter_pfb_arms = 32;
    auto rrc_taps_pfb = firdes::root_raised_cosine(static_cast<double>(symbol_filter_pfb_arms) / static_cast<double>(norm),
                                                   static_cast<double>(symbol_filter_pfb_arms * samples_per_symbol), 1.0,
                                                   0.35, symbol_filter_pfb_arms * samples_per_symbol * 11U);
    rrc_taps_pfb.pop_back(); // packet_receiver.hpp:104-108
    auto& symbol_filter = fg.emplaceBlock<SymbolFilter<c64, c64, float>>({ { "taps", rrc_taps_pfb },
                                                                           { "num_arms", symbol_filter_pfb_arms },
                                                                           { "samples_per_symbol", samples_per_symbol },
                                                                           { "delay", rrc_taps.size() - 1 } });
    std::vector<float> syncword_bipolar;
    for (auto b : syncword) syncword_bipolar.push_back(b ? -1.0f : 1.0f);
    auto& syncword_wipeoff = fg.emplaceBlock<SyncwordWipeoff<>>({ { "syncword", syncword_bipolar } });
    // the front-end test feeds no constellation tags: the loop runs the payload's constellation throughout
    auto& costas_loop = fg.emplaceBlock<CostasLoop<>>({ { "constellation", "QPSK" } });
    {   // a key the block does not have is an error, as in the runtime
        bool thrown = false;
        try {
            fg.emplaceBlock<CoarseFrequencyCorrection<>>({ { "no_such_setting", 1 } });
        } catch (const gr::exception&) {
            thrown = true;
        }
        if (!thrown) throw std::runtime_error("emplaceBlock accepted an unknown setting");
    }
    for (bool* ho : { &syncword_detection.host_output, &syncword_filter.host_output, &freq_correction.host_output,
                      &symbol_filter.host_output, &syncword_wipeoff.host_output })
        *ho = host_output; // internal edges; the last block always writes the host span
    costas_loop.host_output = true;
    if (tail) syncword_wipeoff.host_output = true; // (the tail's edges are dumped: every tail block writes its host span)
    // ---- behind the front end, exactly as packet_receiver.hpp:123-139 creates them (the literal keys and values)
    const std::string packet_len_tag_key = "packet_len";
    const bool log = false;
    auto& payload_metadata_insert = fg.emplaceBlock<PayloadMetadataInsert<>>({ { "log", log } });
    auto& tail_costas_loop = fg.emplaceBlock<CostasLoop<>>();
    auto& syncword_remove = fg.emplaceBlock<SyncwordRemove<>>();
    auto& constellation_decoder =
        fg.emplaceBlock<ConstellationLLRDecoder<>>({ { "noise_sigma", 0.7f }, { "constellation", "QPSK" } });
    auto& descrambler = fg.emplaceBlock<AdditiveScrambler<float>>({ { "mask", uint64_t{ 0x4001U } },
                                                                    { "seed", uint64_t{ 0x18E38U } },
                                                                    { "length", uint64_t{ 16U } },
                                                                    { "reset_tag_key", "header_start" } });
    auto& header_payload_split = fg.emplaceBlock<HeaderPayloadSplit<>>({ { "packet_len_tag_key", packet_len_tag_key } });
    auto& header_fec_decoder = fg.emplaceBlock<HeaderFecDecoder>();
    auto& symbols_split = fg.emplaceBlock<HeaderPayloadSplit<c64>>( // :159-162 (zmq_output)
        { { "header_size", size_t{ 128 } }, { "payload_length_key", "payload_symbols" } });

    syncword_detection.start();
    syncword_filter.start();
    freq_correction.start();
    symbol_filter.start();
    syncword_wipeoff.start();
    if (tail) {
        payload_metadata_insert.start();
        syncword_remove.start();
        descrambler.start();
        header_payload_split.start();
        header_fec_decoder.start();
        symbols_split.start();
    }
    const size_t n_sym_cap = x.size() / sps + 64;
    Edge<c64> e_pm(n_sym_cap), e_cl(n_sym_cap), e_sr(n_sym_cap), e_hsym(n_sym_cap), e_psym(n_sym_cap), e_sr2(n_sym_cap);
    Edge<float> e_llr(2 * n_sym_cap), e_ds(2 * n_sym_cap), e_hdr(2 * n_sym_cap), e_pay(2 * n_sym_cap);
    Edge<uint8_t> e_bytes(n_sym_cap);
    std::deque<gr::Message> pm_headers;
    size_t pm_seen_tags = 0, sr_copied = 0;

    Edge<c64> e_in(x.size()), e_sd(x.size()), e_sdf(x.size()), e_cfc(x.size()), e_sym(x.size() / sps + 64),
        e_wipe(x.size() / sps + 64), e_out(x.size() / sps + 64);
    std::copy(x.begin(), x.end(), e_in.data.begin());
    e_in.size = x.size();

    // round-robin over the blocks, one processBulk() each, like a single-threaded scheduler: a block's output
    // is usually consumed before the block runs again (with host_output = 0 it then never touches the host)
    std::deque<gr::Message> headers;
    std::vector<gr::Message> ignored;
    size_t seen_tags = 0;
    for (int guard = 0; guard < 10000000; ++guard) {
        bool progress = false;
        progress |= step(syncword_detection, e_in, e_sd, max_chunk,
                         [&](auto& is, auto& os) { return syncword_detection.processBulk(is, os); });
        // tag gate: every syncword it lets through is answered with a parsed_header message, as the header
        // parser downstream would (packet_receiver.hpp:244-248)
        progress |= step(syncword_filter, e_sd, e_sdf, max_chunk, [&](auto& is, auto& os) {
            std::vector<gr::Message> hv(headers.begin(), headers.end());
            gr::InSpan<gr::Message> hs(hv.data(), hv.size()), igs(ignored.data(), 0);
            const auto st = syncword_filter.processBulk(hs, igs, is, os);
            for (size_t i = 0; i < hs.consumed; ++i) headers.pop_front();
            if (hs.consumed) progress = true;
            return st;
        });
        for (; seen_tags < e_sdf.tags.size(); ++seen_tags)
            if (e_sdf.tags[seen_tags].map.contains("syncword_amplitude")) {
                headers.push_back({ gr::property_map{ { "packet_length", packet_length } } });
                progress = true;
            }
        progress |= step(freq_correction, e_sdf, e_cfc, max_chunk, [&](auto& is, auto& os) { return freq_correction.processBulk(is, os); });
        progress |= step(symbol_filter, e_cfc, e_sym, max_chunk, [&](auto& is, auto& os) { return symbol_filter.processBulk(is, os); });
        progress |= step(syncword_wipeoff, e_sym, e_wipe, max_chunk, [&](auto& is, auto& os) { return syncword_wipeoff.processBulk(is, os); });
        if (!tail)
            progress |= step(costas_loop, e_wipe, e_out, max_chunk, [&](auto& is, auto& os) { return costas_loop.processBulk(is, os); });
        if (tail) {
            // every syncword that reaches PayloadMetadataInsert is answered with its parsed_header message, as the
            // header parser does (packet_receiver.hpp:241-243)
            for (; pm_seen_tags < e_wipe.tags.size(); ++pm_seen_tags)
                if (e_wipe.tags[pm_seen_tags].map.contains("syncword_amplitude")) {
                    pm_headers.push_back({ gr::property_map{ { "packet_length", packet_length } } });
                    progress = true;
                }
            progress |= step(payload_metadata_insert, e_wipe, e_pm, max_chunk, [&](auto& is, auto& os) {
                std::vector<gr::Message> hv(pm_headers.begin(), pm_headers.end()), ign(4);
                gr::InSpan<gr::Message> hs(hv.data(), hv.size());
                gr::OutSpan<gr::Message> igs(ign.data(), ign.size());
                const auto st = payload_metadata_insert.processBulk(hs, is, os, igs);
                for (size_t i = 0; i < hs.consumed; ++i) pm_headers.pop_front();
                if (hs.consumed) progress = true;
                return st;
            });
            progress |= step(tail_costas_loop, e_pm, e_cl, max_chunk, [&](auto& is, auto& os) { return tail_costas_loop.processBulk(is, os); });
            progress |= step(syncword_remove, e_cl, e_sr, max_chunk, [&](auto& is, auto& os) { return syncword_remove.processBulk(is, os); });
            // SyncwordRemove's output has two readers (:159-162,216-219): the second one reads a copy of the edge
            for (; sr_copied < e_sr.size; ++sr_copied) e_sr2.data[sr_copied] = e_sr.data[sr_copied];
            e_sr2.size = e_sr.size;
            e_sr2.tags = e_sr.tags;
            progress |= step(constellation_decoder, e_sr, e_llr, max_chunk, [&](auto& is, auto& os) { return constellation_decoder.processBulk(is, os); });
            progress |= step(descrambler, e_llr, e_ds, max_chunk, [&](auto& is, auto& os) { return descrambler.processBulk(is, os); });
            progress |= step_split(header_payload_split, e_ds, e_hdr, e_pay, max_chunk);
            progress |= step(header_fec_decoder, e_hdr, e_bytes, max_chunk, [&](auto& is, auto& os) { return header_fec_decoder.processBulk(is, os); });
            progress |= step_split(symbols_split, e_sr2, e_hsym, e_psym, max_chunk);
        }
        if (!progress) break;
    }
    const std::vector<gr::Tag> sd_tags = e_sd.tags;
    // every tag that went into the symbol filter has come out again (the stream ends in zeros), so the wrapper holds no
    // property_map any more (it used to keep one per tag for the life of the block)
    if (symbol_filter.held_tag_maps() != 0)
        throw std::runtime_error("SymbolFilter wrapper still holds " + std::to_string(symbol_filter.held_tag_maps()) + " tag maps");

    if (tail) {
        dump(prefix + ".pm.c64", e_pm.data.data(), e_pm.size);
        dump(prefix + ".costas.c64", e_cl.data.data(), e_cl.size);
        dump(prefix + ".data.c64", e_sr.data.data(), e_sr.size);
        dump(prefix + ".llr.f32", e_llr.data.data(), e_llr.size);
        dump(prefix + ".hdr_llr.f32", e_hdr.data.data(), e_hdr.size);
        dump(prefix + ".pay_llr.f32", e_pay.data.data(), e_pay.size);
        dump(prefix + ".hdr_bytes.u8", e_bytes.data.data(), e_bytes.size);
        dump(prefix + ".hdr_sym.c64", e_hsym.data.data(), e_hsym.size);
        dump(prefix + ".pay_sym.c64", e_psym.data.data(), e_psym.size);
        std::vector<uint64_t> pay_tag_idx, hdr_invalid;
        for (const auto& t : e_pay.tags) pay_tag_idx.push_back(static_cast<uint64_t>(t.index));
        for (const auto& t : e_bytes.tags)
            if (t.map.contains("invalid_header")) hdr_invalid.push_back(static_cast<uint64_t>(t.index));
        dump(prefix + ".pay_tag_index.u64", pay_tag_idx.data(), pay_tag_idx.size());
        const uint64_t tc[8] = { e_pm.size, e_cl.size, e_sr.size, e_llr.size, e_hdr.size, e_pay.size, e_bytes.size, hdr_invalid.size() };
        dump(prefix + ".tail_counts.bin", tc, 8);
        std::printf("receiver tail: pm %zu (tags %zu) data %zu llr %zu header llr %zu payload llr %zu header bytes %zu (invalid %zu) "
                    "symbol split %zu + %zu\n", e_pm.size, e_pm.tags.size(), e_sr.size, e_llr.size, e_hdr.size, e_pay.size,
                    e_bytes.size, hdr_invalid.size(), e_hsym.size, e_psym.size);
    }
    dump(prefix + ".symbols.c64", e_out.data.data(), e_out.size);
    dump_tags(prefix + ".sd_tags.bin", sd_tags);
    dump_tags(prefix + ".sym_tags.bin", e_sym.tags);
    const uint64_t counts[4] = { e_sd.size, e_sdf.size, e_sym.size, e_out.size };
    dump(prefix + ".counts.bin", counts, 4);
    if (host_output) dump(prefix + ".sd.c64", e_sd.data.data(), e_sd.size);
    std::printf("chain: in %zu sd %zu (tags %zu) gate %zu symbols %zu (tags %zu) out %zu\n", x.size(), e_sd.size,
                sd_tags.size(), e_sdf.size, e_sym.size, e_sym.tags.size(), e_out.size);
    return 0;
}

static int blocks(int argc, char** argv)
{
    if (argc < 4) return 2;
    const auto x = read_c64(argv[2]);
    const std::string prefix = argv[3];
    Edge<c64> e_in(x.size()), e_rot(x.size()), e_fir(4 * x.size() + 64), e_arb(8 * x.size() + 64);
    std::copy(x.begin(), x.end(), e_in.data.begin());
    e_in.size = x.size();
    gr::stub::Graph fg;
    auto& rot = fg.emplaceBlock<Rotator<>>({ { "phase_incr", 0.1f } }); // qa_rotator.cpp:20
    rot.start();
    run(rot, e_in, e_rot, 5000, [&](auto& is, auto& os) { return rot.processBulk(is, os); });
    auto& fir = fg.emplaceBlock<InterpolatingFirFilter<c64, c64, float>>(
        { { "interpolation", size_t{ 4 } }, { "taps", firdes::root_raised_cosine(1.0, 4.0, 1.0, 0.35, 44) } });
    run(fir, e_rot, e_fir, 3001, [&](auto& is, auto& os) { return fir.processBulk(is, os); });
    std::vector<float> arb_taps(1280);
    {
        FILE* f = std::fopen(argv[4], "rb"); // the default taps (data/pfb_arb_taps.f32)
        if (!f) throw std::runtime_error("cannot read taps");
        if (std::fread(arb_taps.data(), 4, 1280, f) != 1280) throw std::runtime_error("short taps");
        std::fclose(f);
    }
    auto& arb = fg.emplaceBlock<PfbArbResampler<c64, c64, float, double>>( // qa_pfb_arb_resampler.cpp:28-31
        { { "rate", 1.1234 }, { "taps", arb_taps } });
    run(arb, e_fir, e_arb, 7001, [&](auto& is, auto& os) { return arb.processBulk(is, os); });
    dump(prefix + ".rot.c64", e_rot.data.data(), e_rot.size);
    dump(prefix + ".fir.c64", e_fir.data.data(), e_fir.size);
    dump(prefix + ".arb.c64", e_arb.data.data(), e_arb.size);
    std::printf("blocks: rot %zu fir %zu arb %zu\n", e_rot.size, e_fir.size, e_arb.size);
    return 0;
}


// test/qa_symbol_filter.cpp:17-63 on the wrappers: +-1 float symbols -> InterpolatingFirFilter<float, float, float> (4 x,
// 44-tap RRC) -> SymbolFilter<float, float, float> (32 arms); ragged chunk sizes
static std::vector<float> read_f32(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    std::fseek(f, 0, SEEK_END);
    const size_t n = static_cast<size_t>(std::ftell(f)) / sizeof(float);
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> x(n);
    if (n && std::fread(x.data(), sizeof(float), n, f) != n) throw std::runtime_error("short read");
    std::fclose(f);
    return x;
}
static int floats(int argc, char** argv)
{
    if (argc < 4) return 2;
    const auto x = read_f32(argv[2]);
    const std::string prefix = argv[3];
    const size_t sps = 4, arms = 32;
    Edge<float> e_in(x.size()), e_fir(sps * x.size() + 64), e_sym(x.size() + 64);
    std::copy(x.begin(), x.end(), e_in.data.begin());
    e_in.size = x.size();
    gr::stub::Graph fg;
    auto& fir = fg.emplaceBlock<InterpolatingFirFilter<float, float, float>>(
        { { "interpolation", sps }, { "taps", firdes::root_raised_cosine(1.0, static_cast<double>(sps), 1.0, 0.35, sps * 11) } });
    run(fir, e_in, e_fir, 2999, [&](auto& is, auto& os) { return fir.processBulk(is, os); });
    auto& symf = fg.emplaceBlock<SymbolFilter<float, float, float>>(
        { { "taps", firdes::root_raised_cosine(static_cast<double>(arms), static_cast<double>(arms * sps), 1.0, 0.35, arms * sps * 11) },
          { "num_arms", arms },
          { "samples_per_symbol", sps } });
    symf.start();
    run(symf, e_fir, e_sym, 10007, [&](auto& is, auto& os) { return symf.processBulk(is, os); });
    dump(prefix + ".fir.f32", e_fir.data.data(), e_fir.size);
    dump(prefix + ".sym.f32", e_sym.data.data(), e_sym.size);
    std::printf("floats: fir %zu symbols %zu\n", e_fir.size, e_sym.size);
    return 0;
}

// gr::packet_modem::Pdu<T> by shape (pdu.hpp:15-21; the reference's header is not on the GPU box)
template <typename T>
struct TestPdu {
    using value_type = T;
    std::vector<T> data{};
    std::vector<gr::Tag> tags{};
};
static int pdus(int argc, char** argv)
{
    if (argc < 5) return 2;
    std::vector<uint8_t> bits;
    {
        FILE* f = std::fopen(argv[2], "rb");
        if (!f) throw std::runtime_error("cannot read bits");
        std::fseek(f, 0, SEEK_END);
        bits.resize(static_cast<size_t>(std::ftell(f)));
        std::fseek(f, 0, SEEK_SET);
        if (!bits.empty() && std::fread(bits.data(), 1, bits.size(), f) != bits.size()) throw std::runtime_error("short read");
        std::fclose(f);
    }
    const auto sym = read_c64(argv[3]);
    const std::string prefix = argv[4];
    gr::stub::Graph fg;
    // packet_transmitter_pdu.hpp:119-122: the CCSDS scrambler, restarted at the head of every PDU
    auto& scr = fg.emplaceBlock<AdditiveScrambler<TestPdu<uint8_t>>>(
        { { "mask", uint64_t{ 0x4001U } }, { "seed", uint64_t{ 0x18E38U } }, { "length", uint64_t{ 16U } } });
    scr.start();
    std::vector<uint8_t> scr_out;
    std::vector<uint64_t> sizes, fir_sizes;
    uint32_t lcg = 12345u;
    auto next_size = [&](size_t left) {
        lcg = lcg * 1664525u + 1013904223u;
        const size_t want = (lcg >> 16) % 5 == 0 ? 0 : 1 + (lcg >> 8) % 4000; // every fifth PDU is empty
        return std::min(want, left);
    };
    for (size_t pos = 0; pos < bits.size();) {
        const size_t n = next_size(bits.size() - pos);
        TestPdu<uint8_t> pdu;
        pdu.data.assign(bits.begin() + static_cast<ssize_t>(pos), bits.begin() + static_cast<ssize_t>(pos + n));
        pdu.tags.push_back({ 0, { { "packet_len", static_cast<uint64_t>(n) } } });
        const auto out = scr.processOne(pdu);
        if (out.data.size() != n || out.tags.size() != 1 || out.tags[0].index != 0) throw std::runtime_error("scrambler PDU shape");
        scr_out.insert(scr_out.end(), out.data.begin(), out.data.end());
        sizes.push_back(n);
        pos += n;
    }
    // packet_transmitter_pdu.hpp:288-291: the RRC interpolator on symbol PDUs, history running on across PDUs
    auto& fir = fg.emplaceBlock<InterpolatingFirFilter<TestPdu<c64>, TestPdu<c64>, float>>(
        { { "interpolation", size_t{ 4 } }, { "taps", firdes::root_raised_cosine(1.0, 4.0, 1.0, 0.35, 44) } });
    std::vector<c64> fir_out;
    std::vector<uint64_t> tag_index;
    for (size_t pos = 0; pos < sym.size();) {
        const size_t n = next_size(sym.size() - pos);
        TestPdu<c64> pdu;
        pdu.data.assign(sym.begin() + static_cast<ssize_t>(pos), sym.begin() + static_cast<ssize_t>(pos + n));
        if (n) pdu.tags.push_back({ static_cast<ssize_t>(n / 2), { { "mark", static_cast<uint64_t>(pos) } } });
        const auto out = fir.processOne(pdu);
        if (out.data.size() != 4 * n || out.tags.size() != pdu.tags.size()) throw std::runtime_error("FIR PDU shape");
        for (const auto& t : out.tags) tag_index.push_back(fir_out.size() + static_cast<uint64_t>(t.index)); // :167-171
        fir_out.insert(fir_out.end(), out.data.begin(), out.data.end());
        fir_sizes.push_back(n);
        pos += n;
    }
    dump(prefix + ".scr.u8", scr_out.data(), scr_out.size());
    dump(prefix + ".fir.c64", fir_out.data(), fir_out.size());
    dump(prefix + ".scr_sizes.u64", sizes.data(), sizes.size());
    dump(prefix + ".fir_sizes.u64", fir_sizes.data(), fir_sizes.size());
    dump(prefix + ".fir_tag_index.u64", tag_index.data(), tag_index.size());
    std::printf("pdus: %zu + %zu PDUs, scrambled %zu, filtered %zu\n", sizes.size(), fir_sizes.size(), scr_out.size(), fir_out.size());
    return 0;
}

// ZmqPduPubSink<c64> as PacketReceiver wires it (packet_receiver.hpp:163-168), on an ephemeral port
static int zmq_mode(int argc, char** argv)
{
    if (argc < 3) return 2;
    const int n_pdus = std::atoi(argv[2]);
    gr::stub::Graph fg;
    auto& sink = fg.emplaceBlock<ZmqPduPubSink<c64>>({ { "endpoint", "tcp://127.0.0.1:*" } });
    sink.start();
    std::printf("port %d\n", sink.port());
    std::fflush(stdout);
    for (int i = 0; i < 5000 && sink.subscribers() == 0; ++i) std::this_thread::sleep_for(std::chrono::milliseconds(2));
    if (sink.subscribers() == 0) throw std::runtime_error("no subscriber came");
    for (int k = 0; k < n_pdus; ++k) {
        gr::packet_modem::Pdu<c64> pdu;
        pdu.data.resize(k % 3 == 0 ? 128 : 100 + 37 * static_cast<size_t>(k));
        for (size_t i = 0; i < pdu.data.size(); ++i) pdu.data[i] = c64(static_cast<float>(k), static_cast<float>(i));
        sink.processOne(pdu);
    }
    sink.stop(); // (what is queued gets its linger time)
    std::printf("published %d\n", n_pdus);
    return 0;
}

// HeaderFecDecoder::start() with the alist text of a file: the block is built for the header code's 256 LLRs -> 4 bytes
// and refuses (gr::exception, exit status 1 through main) every other code the decoder itself accepts
static int fec_alist(int argc, char** argv)
{
    if (argc < 3) return 2;
    std::ifstream f(argv[2]);
    if (!f) return 2;
    std::stringstream ss;
    ss << f.rdbuf();
    gr::stub::Graph fg;
    auto& dec = fg.emplaceBlock<HeaderFecDecoder>();
    dec.alist = ss.str();
    dec.start();
    dec.stop();
    std::printf("started\n");
    return 0;
}

// A double-mapped ring between two wrapped blocks with host_output = false (gnuradio4's CircularBuffer maps its storage
// twice, back to back): the producer's spans run past the end of the first mapping, the consumer -- reading in smaller
// chunks -- sees the items behind the wrap at addresses one ring size lower.  The host memory of the ring is never
// written here (host_output = false) and is filled with NaNs: the consumer gets correct data only from the device
// arena, i.e. only if the arena compares addresses modulo the registered ring.
static int mirror(int argc, char** argv)
{
    if (argc < 4) return 2;
    const auto x = read_c64(argv[2]);
    const std::string prefix = argv[3];
    const size_t R = 4096; // ring size in items
    std::vector<c64> ring(2 * R, c64{ std::nanf(""), std::nanf("") });
    gr::packet_modem::hip::detail::Arena::instance().add_mirrored_ring(ring.data(), R * sizeof(c64));
    gr::stub::Graph fg;
    auto& a = fg.emplaceBlock<Rotator<>>({ { "phase_incr", 0.1f } });
    auto& b = fg.emplaceBlock<Rotator<>>({ { "phase_incr", -0.03f } });
    a.host_output = false;
    b.host_output = true;
    a.start();
    b.start();
    std::vector<c64> out(x.size());
    size_t in_pos = 0, w = 0, r = 0, o = 0; // items read from x, written to / read from the ring, written to out
    const size_t prod_chunk[3] = { 1500, 2900, 777 }, cons_chunk[2] = { 640, 1111 };
    std::vector<std::pair<size_t, size_t>> spans; // producer spans [begin, end) in item counts, for the consumer to stay inside
    size_t pi = 0, ci = 0, hits_needed = 0;
    while (o < x.size()) {
        // producer: as much as fits (never more than R items ahead of the reader)
        const size_t room = R - (w - r);
        size_t np = std::min({ prod_chunk[pi % 3], x.size() - in_pos, room });
        if (np > 0) {
            gr::InSpan<c64> is(x.data() + in_pos, np);
            gr::OutSpan<c64> os(ring.data() + (w % R), np); // may run into the second mapping
            if (a.processBulk(is, os) != gr::work::Status::OK) throw std::runtime_error("producer");
            in_pos += is.consumed;
            spans.push_back({ w, w + os.published });
            w += os.published;
            ++pi;
        }
        // consumer: chunks that stay inside one producer span
        while (r < w) {
            size_t end = w;
            for (const auto& sp : spans)
                if (r >= sp.first && r < sp.second) end = sp.second;
            const size_t nc = std::min(cons_chunk[ci % 2], end - r);
            gr::InSpan<c64> is(ring.data() + (r % R), nc); // after the wrap: one ring size below the producer's address
            gr::OutSpan<c64> os(out.data() + o, nc);
            if (b.processBulk(is, os) != gr::work::Status::OK) throw std::runtime_error("consumer");
            if ((r % R) + nc <= R && (r / R) != ((spans.back().first) / R)) ++hits_needed;
            r += is.consumed;
            o += os.published;
            ++ci;
        }
    }
    dump(prefix + ".mirror.c64", out.data(), out.size());
    std::printf("mirror: %zu items through a %zu-item double-mapped ring, %zu consumer spans behind a wrap\n", o, R, hits_needed);
    return 0;
}

// The same double-mapped ring with the two ends of the edge in TWO THREADS (the reference's multi-threaded schedulers,
// benchmarks/README.md:8-26): the producer runs ahead as far as the ring allows while the consumer is still inside the
// spans before.  host_output = false and NaNs in the host ring: every consumer span has to come from a device buffer
// the producer has not reused in the meantime (the arena's pool and pins), or from the write-back of a retired one.
static int threads(int argc, char** argv)
{
    if (argc < 4) return 2;
    const auto x = read_c64(argv[2]);
    const std::string prefix = argv[3];
    const size_t R = 8192; // ring size in items (64 KiB: whole pages)
    // a REAL double mapping, as gnuradio4's CircularBuffer makes it (one memfd mapped twice, back to back): when the
    // arena writes the unconsumed rest of a retired span back through the producer's address, the consumer sees it
    // through the other mapping
    const int fd = memfd_create("gr4pm_ring", 0);
    if (fd < 0 || ftruncate(fd, static_cast<off_t>(R * sizeof(c64))) != 0) throw std::runtime_error("memfd");
    char* base = static_cast<char*>(mmap(nullptr, 2 * R * sizeof(c64), PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
    if (base == MAP_FAILED) throw std::runtime_error("mmap reserve");
    for (int k = 0; k < 2; ++k)
        if (mmap(base + k * R * sizeof(c64), R * sizeof(c64), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_FIXED, fd, 0) == MAP_FAILED)
            throw std::runtime_error("mmap ring");
    c64* ring_p = reinterpret_cast<c64*>(base);
    for (size_t i = 0; i < R; ++i) ring_p[i] = c64{ std::nanf(""), std::nanf("") };
    struct RingView {
        c64* p;
        c64* data() const { return p; }
    } ring{ ring_p };
    gr::packet_modem::hip::detail::Arena::instance().add_mirrored_ring(ring.data(), R * sizeof(c64));
    gr::stub::Graph fg;
    auto& a = fg.emplaceBlock<Rotator<>>({ { "phase_incr", 0.1f } });
    auto& b = fg.emplaceBlock<Rotator<>>({ { "phase_incr", -0.03f } });
    a.host_output = false;
    b.host_output = true;
    a.start();
    b.start();
    std::vector<c64> out(x.size());
    std::atomic<size_t> w{ 0 }, r{ 0 }; // items written to / read from the ring
    std::mutex m;
    std::vector<std::pair<size_t, size_t>> spans; // producer spans, for the consumer to stay inside one
    std::atomic<bool> failed{ false };
    size_t ahead_max = 0;
    std::thread producer([&] {
        try {
            const size_t chunk[4] = { 1500, 2900, 777, 2048 };
            size_t in_pos = 0, k = 0;
            while (in_pos < x.size() && !failed) {
                const size_t room = R - (w.load() - r.load(std::memory_order_acquire));
                const size_t np = std::min({ chunk[k % 4], x.size() - in_pos, room });
                if (np == 0) {
                    std::this_thread::yield();
                    continue;
                }
                gr::InSpan<c64> is(x.data() + in_pos, np);
                gr::OutSpan<c64> os(ring.data() + (w.load() % R), np);
                if (a.processBulk(is, os) != gr::work::Status::OK) throw std::runtime_error("producer");
                in_pos += is.consumed;
                {
                    std::lock_guard<std::mutex> g(m);
                    spans.push_back({ w.load(), w.load() + os.published });
                }
                w.store(w.load() + os.published, std::memory_order_release);
                ++k;
            }
        } catch (const std::exception& e) {
            std::fprintf(stderr, "producer: %s\n", e.what());
            failed = true;
        }
    });
    try {
        const size_t chunk[3] = { 640, 1111, 333 };
        size_t o = 0, k = 0;
        while (o < x.size() && !failed) {
            const size_t wr = w.load(std::memory_order_acquire), rd = r.load();
            if (rd == wr) {
                std::this_thread::yield();
                continue;
            }
            ahead_max = std::max(ahead_max, wr - rd);
            size_t end = wr;
            {
                std::lock_guard<std::mutex> g(m);
                for (const auto& sp : spans)
                    if (rd >= sp.first && rd < sp.second) end = sp.second;
            }
            const size_t nc = std::min(chunk[k % 3], end - rd);
            gr::InSpan<c64> is(ring.data() + (rd % R), nc);
            gr::OutSpan<c64> os(out.data() + o, nc);
            if (b.processBulk(is, os) != gr::work::Status::OK) throw std::runtime_error("consumer");
            r.store(rd + is.consumed, std::memory_order_release);
            o += os.published;
            ++k;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "consumer: %s\n", e.what());
        failed = true;
    }
    producer.join();
    if (failed) return 1;
    dump(prefix + ".threads.c64", out.data(), out.size());
    const auto lk = gr::packet_modem::hip::detail::Arena::instance().lookups();
    std::printf("threads: %zu items through a %zu-item double-mapped ring, producer up to %zu items ahead, device hits %zu "
                "uploads %zu\n", out.size(), R, ahead_max, lk.first, lk.second);
    return 0;
}

int main(int argc, char** argv)
{
    try {
        if (argc >= 2 && std::strcmp(argv[1], "chain") == 0) return chain(argc, argv);
        if (argc >= 2 && std::strcmp(argv[1], "receiver") == 0) return chain(argc, argv, true);
        if (argc >= 2 && std::strcmp(argv[1], "blocks") == 0) return blocks(argc, argv);
        if (argc >= 2 && std::strcmp(argv[1], "floats") == 0) return floats(argc, argv);
        if (argc >= 2 && std::strcmp(argv[1], "pdus") == 0) return pdus(argc, argv);
        if (argc >= 2 && std::strcmp(argv[1], "zmq") == 0) return zmq_mode(argc, argv);
        if (argc >= 2 && std::strcmp(argv[1], "mirror") == 0) return mirror(argc, argv);
        if (argc >= 2 && std::strcmp(argv[1], "threads") == 0) return threads(argc, argv);
        if (argc >= 2 && std::strcmp(argv[1], "fec_alist") == 0) return fec_alist(argc, argv);
        std::fprintf(stderr, "usage: %s chain|receiver|blocks|mirror|threads|fec_alist ...\n", argv[0]);
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "gr4_blocks_driver: %s\n", e.what());
        return 1;
    }
}
