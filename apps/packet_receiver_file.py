#!/usr/bin/env python3
"""MI355X counterpart of the reference's apps/packet_receiver_file.cpp (apps/README.md:5-24):

    packet_receiver_file.py input_file [syncword_freq_bins=4] [syncword_threshold=9.5] [--out packets.bin] [--zmq]
                            [--format {cf32,sc16,sc8,cu8}] [--scale S] [--tune CYCLES_PER_SAMPLE|auto --decimate N[/M]]
                            [--refine] [--decimate auto] [--burst-rows] [--fft-ddc] [--notch F:BW ...] [--notch-taps N]
                            [--scan [--scan-items N] [--bursts] [--waterfall FILE.npy [--waterfall-average R]]]

reads IQ samples from `input_file` in raw little-endian complex64 (std::complex<float>, what
FileSource<c64> freads, file_source.hpp:32,53) at 4 samples/symbol, runs the whole receiver on
the GPU (gr4pm_packet_receiver, decode_headers: detection ... header decode ... CRC check) and
hands over the packets whose CRC-32 matches.  The reference writes them to a TUN device (needs
root and a network namespace); here they go to `--out` as records of a big-endian uint16 length
followed by the bytes, or are just counted.

`--zmq` is the reference app's `zmq_output = true` (apps/packet_receiver_file.cpp, packet_receiver.hpp:159-189): the
header symbols of every packet are published as one ZeroMQ message of raw complex64 on tcp port 5000 and the payload
symbols on 5001 (`--zmq-ports H P` for others), where scripts/plot_symbols.py of the reference connects its SUB sockets;
the library speaks the ZeroMQ wire protocol itself (gr4pm_zmq_pub_*), libzmq is not needed.

`--format sc16 | sc8 | cu8`: the file holds interleaved little-endian int16, int8 or uint8 (I, Q) instead (an SDR
driver's buffers, SigMF ci16_le / ci8, rtl_sdr's cu8).  It crosses the host link as it is, 4 or 2 bytes per sample, and
becomes complex64 on the device (gr4pm_iq_unpack, `--scale`: per component, default 2^-15 or 2^-7).

`--tune F --decimate D`: the file is a wideband recording with the modem's carrier F cycles per file sample off centre
and D times the modem's rate: it goes through a one-channel `Ddc` (gr4pm_ddc: mix by -F, low-pass, keep every D-th
sample) in front of the receiver.  Combines with `--format` (the Ddc reads the integers itself).  The
counts are then in samples at the receiver's rate.  `--decimate N/M` (N >= M, for instance 25/4 for a 25 Msps file of a
1 Msym/s carrier): N / M file samples per receiver sample, the same Ddc resampling by M / N in the same pass (DESIGN
section 18), so any symbol rate lands on the receiver's 4 samples per symbol.

`--scan [--scan-items N]`: where are the carriers?  The first N items of the file (default: all) go through a `Spectrum`
(gr4pm_spectrum: Welch PSD of 2048 bins with a running maximum per bin; `--format` / `--scale` as
above), `find_carriers` reads the maximum-hold spectrum, and the app prints one line per carrier (frequency in cycles
per file sample, bandwidth, snr_db) and exits.  `--tune auto` runs the same scan and tunes to the carrier of greatest
power.  A scan resolves one bin, 1 / 2048 cycles per sample; the detector behind the Ddc pulls in +-0.00673 / D, so
`--decimate` of at most 13 keeps a bin inside it.

`--scan --bursts`: and when are they on the air?  After the carrier lines the scanned items go through a `Spectrogram`
(gr4pm_spectrogram: PSD rows over time, hop 1024) chunk by chunk; the power of every carrier's band
(`band_power`, on the device) is appended per chunk on the host, `find_bursts` reads each carrier's series, and the app
prints one line per burst: `burst frequency F start S end E snr_db X`, S and E (exclusive) in file samples, a burst's
edges being as fine as a row (`--waterfall-average` rows of hop 1024, 2048 samples wide).  `--waterfall FILE.npy` writes
the rows of the scanned items (float32 [rows, 2048], FFT bin order, mean of `--waterfall-average` R segments per row,
default 1) for a waterfall plot.  `--scan` alone prints what it always printed.

`--refine` (with `--tune`, a value or `auto`) and `--decimate auto`: the blind receiver.  The first `--scan-items` items
(at most one chunk) are scanned as above; the tuned carrier's bursts (`Spectrogram`, `find_bursts`) are down-converted
on their own at a provisional decimation of floor(0.4 / bandwidth) (`Ddc.extract`), and a `LineSpectrum` (DESIGN section
23) reads from those rows the residual carrier offset (the line of x^4) and the symbol rate (the line of |x|^2), both
the median over the rows whose carrier line stands 6 dB above everything else it was searched among.  `--refine` adds
the offset to the tuned frequency and prints it; `--decimate auto` turns the rate into the simplest N/M that puts 4
samples on a symbol (`resample_ratio`), prints it and uses it.

`--burst-rows` (with `--tune` and `--decimate`, each a value or `auto`): the burst chain to the end.  The file, which has
to fit one chunk (`--chunk-items`), is scanned, the tuned carrier's bursts are extracted at the provisional decimation
and read by the `LineSpectrum` as above, and a `RowResampler` brings every burst row to 4 samples per
symbol and removes its residual offset ON THE ROWS, each row with its own measured rate (`--decimate auto`) or the typed
N/M, and its own offset; a row whose carrier line stands less than 6 dB above the rest takes the carrier's medians.  The
receiver takes the rows.  No streaming `Ddc` runs over the file, and the rate need not be a simple fraction.  If no row
shows a carrier line, the app says so and falls back to the streaming path.

`--notch F:BW` (repeatable), `--notch-taps N` (odd, default 1025): the band BW cycles per file sample wide around F is
removed from the file's samples before anything else sees them: a CW interferer inside the channel, the DC spike of an
rtl_sdr recording (`--notch 0:0.004`), a strong neighbour.  The bands become one band-stop design (`band_filter_taps`, 60
dB) in an `FftFilter` (gr4pm_fft_filter: fast convolution) in front of the plain receiver, of `--tune`
and of `--fft-ddc`; it reads the file's format itself and is flushed at the end of the file, so as many samples come out
as went in, delayed by (N - 1) / 2.  It goes with none of the scanning options (`--scan`, `--tune auto`, `--refine`,
`--decimate auto`, `--burst-rows`), which look at the file as it is.

The file is streamed: host chunks are staged in pinned memory and copied to the device on a
copy stream while the previous chunk is being processed; the samples the detector leaves
unconsumed (less than one FFT block) are presented again in front of the next chunk."""
import argparse
import os
import sys
import time

# A recording is mostly silence between packets: the stretch between two detections is one serial phasor chain, and the
# library runs the chains of consecutive batches side by side where the HIP runtime has hardware queues to spare
# ("Process settings"; read when the runtime starts, i.e. before torch is imported)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


FILE_DTYPES = {"cf32": torch.complex64, "sc16": torch.int16, "sc8": torch.int8, "cu8": torch.uint8}


def decimation(v):
    """--decimate: `N` or `N/M`, file samples per receiver sample, as (N, M); an integer passes as (N, 1)"""
    n, _, m = str(v).partition("/")
    try:
        n, m = int(n), int(m) if m else 1
    except ValueError:
        raise ValueError(f"--decimate: {v!r} is neither N nor N/M") from None
    if m < 1 or (m > 1 and n < m):
        raise ValueError(f"--decimate: {v!r}: need N >= M >= 1 (file samples per receiver sample)")
    return n, m  # a plain integer goes to the Ddc as it is, which refuses what it cannot take


def file_chunks(path, fmt="cf32", items=None, chunk_items=1 << 24):
    """the file's first `items` items (None: all) as device tensors of at most chunk_items items: complex64 [n], or the
    integers as they are, [n, 2]"""
    file_dtype = FILE_DTYPES[fmt]
    item_bytes = 8 if fmt == "cf32" else 2 * file_dtype.itemsize
    n_file = os.path.getsize(path) // item_bytes
    left = n_file if items is None else min(int(items), n_file)
    with open(path, "rb") as fh:
        while left:
            n = min(left, chunk_items)
            host = torch.empty((n,) if fmt == "cf32" else (n, 2), dtype=file_dtype)
            got = fh.readinto(memoryview(host.numpy().view(np.uint8))) // item_bytes
            if not got:
                break
            yield host[:got].cuda()
            left -= got


def scan_file(path, fmt="cf32", scale=None, items=None, chunk_items=1 << 24, pkg=None):
    """the file's first `items` items (None: all) through a Spectrum: returns (carriers: find_carriers' structured array
    from the maximum-hold spectrum, the Spectrum's read(), items scanned)"""
    pkg = pkg or ge.load_package()
    sp = pkg.Spectrum()
    done = 0
    for x in file_chunks(path, fmt, items, chunk_items):
        sp.process_bulk(x) if fmt == "cf32" else sp.process_bulk(x, scale=scale)
        done += x.shape[0]
    r = sp.read()
    return pkg.find_carriers(r["max_hold"]), r, done


def scan_rows(path, carriers, fmt="cf32", scale=None, items=None, chunk_items=1 << 24, average=1, keep_rows=False, pkg=None):
    """the same items through a Spectrogram (hop 1024, the mean of `average` segments per row), chunk by chunk: returns
    (the Spectrogram, float64 [len(carriers), rows]: the power of every carrier's band per row, the rows themselves as
    float32 [rows, 2048] if keep_rows else None)"""
    pkg = pkg or ge.load_package()
    sg = pkg.Spectrogram(hop=1024, average=average)
    power, rows = [np.zeros((len(carriers), 0))], [np.zeros((0, sg.fft_size), dtype=np.float32)]
    for x in file_chunks(path, fmt, items, chunk_items):
        r = sg.process_bulk(x) if fmt == "cf32" else sg.process_bulk(x, scale=scale)
        if len(carriers):
            power.append(np.concatenate([sg.band_power(r, carriers[i:i + 64]).cpu().numpy()  # a call takes 64 bands
                                         for i in range(0, len(carriers), 64)]))
        if keep_rows:
            rows.append(r.cpu().numpy())
    return sg, np.concatenate(power, axis=1), np.concatenate(rows) if keep_rows else None


def print_bursts(sg, carriers, power):
    for c, p in zip(carriers, power):
        for b in (sg.bursts(p) if p.size else []):
            print(f"burst frequency {c['frequency']:+.6f} start {b['start_sample']} end {b['end_sample']} snr_db {b['snr_db']:.1f}")


def print_carriers(carriers, r, items):
    print(f"{len(carriers)} carriers in {items} items ({r['segments']} segments of 2048, hop 1024)")
    for c in carriers:
        print(f"carrier frequency {c['frequency']:+.6f} bandwidth {c['bandwidth']:.6f} snr_db {c['snr_db']:.1f}")


def decimation_or_auto(v):
    """--decimate: `auto`, or what decimation() takes"""
    return "auto" if str(v).lower() == "auto" else decimation(v)


def burst_rows_of_file(path, tune, bandwidth, fmt="cf32", scale=None, items=None, chunk_items=1 << 24, pkg=None, min_margin_db=6.0):
    """the bursts of the carrier at `tune` (cycles per file sample, `bandwidth` wide) in the file's first min(items,
    chunk_items) items as rows at the provisional decimation, and what a LineSpectrum reads from them: returns
    dict(decimation: D0, rows: the CUDA tensor [R, n] or None without a sample, lengths, offsets: carrier_offset's
    records, good: the rows whose carrier line has margin_db >= min_margin_db, rates: symbol_rate's records, or None when
    no row is good)"""
    pkg = pkg or ge.load_package()
    x = next(file_chunks(path, fmt, items, chunk_items), None)
    if x is None:
        return dict(decimation=1, rows=None, lengths=None, offsets=None, good=None, rates=None)
    kw = {} if fmt == "cf32" else dict(scale=scale)
    d0 = pkg.provisional_decimation(bandwidth)
    ddc = pkg.Ddc([tune], d0, max_frames=-(-x.shape[0] // d0) + 1)
    sg = pkg.Spectrogram(hop=512, average=4)
    half = max(2, int(np.ceil(0.5 * bandwidth * sg.fft_size)))
    band = [((int(round(tune * sg.fft_size)) - half) % sg.fft_size, 2 * half + 1)]
    power = sg.band_power(sg.process_bulk(x, **kw), band)[0]
    found = sg.bursts(power) if power.numel() else []
    if len(found):
        spans = ddc.burst_spans(found, 0, margin_frames=-(-sg.row_span // d0))
        rows, lengths = ddc.extract(x, spans, **kw)
    else:  # no burst stands out (a continuous carrier, or a scan too short to see its floor): the whole stretch as one row
        rows = ddc.process_bulk(x, **kw)
        lengths = np.array([rows.shape[1]], dtype=np.int64)
    # hop 256: a burst may be shorter than a segment, and a dozen placements of it average better than two.  The offset
    # is searched within four bins of the scan (one PSD bin is d0 / 2048 cycles per item): the fewer bins, the fewer
    # chances the self-noise of x^4 has to beat the line
    ls = pkg.LineSpectrum(hop=256)
    max_offset = min(0.1, 4.0 * d0 / sg.fft_size)

    offsets = ls.carrier_offset(rows, lengths, max_offset=max_offset)
    good = offsets["margin_db"] >= min_margin_db  # the rows that show a carrier line: the symbol rate is read from the same
    rates = ls.symbol_rate(rows, lengths) if good.any() else None
    return dict(decimation=d0, rows=rows, lengths=lengths, offsets=offsets, good=good, rates=rates)


def refine_file(path, tune, bandwidth, fmt="cf32", scale=None, items=None, chunk_items=1 << 24, pkg=None, min_margin_db=6.0):
    """the carrier at `tune` (cycles per file sample, `bandwidth` wide) in the file's first min(items, chunk_items) items,
    looked at through a LineSpectrum at the provisional decimation: returns dict(decimation: D0, rows, offset: the median
    residual offset in cycles per FILE sample or None, rate: the median symbol rate in symbols per FILE sample or None);
    only rows whose carrier line has margin_db >= min_margin_db count, for both"""
    b = burst_rows_of_file(path, tune, bandwidth, fmt, scale, items, chunk_items, pkg, min_margin_db)
    if b["rows"] is None:
        return dict(decimation=1, rows=0, offset=None, rate=None)
    d0, good = b["decimation"], b["good"]
    if not good.any():
        return dict(decimation=d0, rows=int(b["rows"].shape[0]), offset=None, rate=None)
    return dict(decimation=d0, rows=int(b["rows"].shape[0]), offset=float(np.median(b["offsets"]["offset"][good])) / d0,
                rate=float(np.median(b["rates"]["rate"][good])) / d0)


def receive_burst_rows(b, syncword_freq_bins=4, syncword_threshold=9.5, rate=None, out=None, pkg=None):
    """burst_rows_of_file()'s rows through a RowResampler to 4 samples per symbol with their residual offsets removed, and
    through the receiver, row by row.  rate: symbols per row item for every row (a typed --decimate), or None: each good
    row's own measured rate.  A row that is not good takes the medians of the good ones, for the rate and for the offset.
    Returns receive_file()'s dict; its items are the resampled rows' items."""
    pkg = pkg or ge.load_package()
    good, offsets = b["good"], b["offsets"]["offset"].copy()
    offsets[~good] = np.median(offsets[good])
    if rate is None:
        rates = b["rates"]["rate"].copy()
        rates[~good] = np.median(rates[good])
    else:
        rates = np.full(offsets.size, float(rate))
    t0 = time.perf_counter()
    rs = pkg.RowResampler()
    # one block of 2048 zeros behind the longest row: the receiver delivers a packet once the block after it has come
    longest = int(rs.output_lengths(b["lengths"], rs.steps_for(rates)).max())
    n_cols = (-(-longest // 2048) + 1) * 2048
    rows, lengths = rs.to_samples_per_symbol(b["rows"], b["lengths"], rates, offsets, n_cols=n_cols)
    packets, stats = [], {"headers": 0, "invalid_headers": 0, "crc_failures": 0}
    for r in range(rows.shape[0]):
        rx = pkg.NativePacketReceiver(4, syncword_freq_bins, syncword_threshold, max_items=n_cols, tags_cap=n_cols // 768 + 64,
                                      decode_headers=True, packets_only=True)
        res = rx.process_bulk(rows[r].contiguous())
        m, lens = res["header_messages"], res["packet_lengths"]
        stats["headers"] += int(m.size)
        stats["invalid_headers"] += int(np.sum(m["invalid_header"] != 0))
        stats["crc_failures"] += int(np.sum(lens == 0))
        data, pos = res["packets"].cpu().numpy(), 0
        for n in lens[lens > 0]:
            packets.append(data[pos:pos + int(n)].tobytes())
            pos += int(n)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if out:
        with open(out, "wb") as f:
            for p in packets:
                f.write(len(p).to_bytes(2, "big"))
                f.write(p)
    items = int(np.sum(lengths))
    return {"packets": packets, "items": items, "file_items": items, "seconds": dt, "rates": rates, "offsets": offsets, **stats}


def notch_band(v):
    """--notch: `F:BW`, centre and width in cycles per file sample, as (F, BW)"""
    f, sep, bw = str(v).partition(":")
    try:
        if not sep:
            raise ValueError
        return float(f), float(bw)
    except ValueError:
        raise ValueError(f"--notch: {v!r} is not F:BW") from None


def tune_value(v):
    """--tune: cycles per file sample, or `auto`"""
    return "auto" if str(v).lower() == "auto" else float(v)


def receive_file(path, syncword_freq_bins=4, syncword_threshold=9.5, chunk_items=1 << 24, out=None, pkg=None, zmq_ports=None,
                 fmt="cf32", scale=None, tune=None, decimate=None, fft_ddc=False, notch=None):
    """returns dict(packets: list of bytes, items, seconds, headers, invalid_headers, crc_failures).  decimate: an
    integer, "N/M" or (N, M).  fft_ddc: an FftDdc in place of the Ddc (a power-of-two decimation).  notch: complex taps
    of an FftFilter in front of everything else (None: none), flushed at the end of the file"""
    pkg = pkg or ge.load_package()
    file_dtype = FILE_DTYPES[fmt]
    shape = (chunk_items,) if fmt == "cf32" else (chunk_items, 2)  # integer IQ: [items, (I, Q)]
    item_bytes = 8 if fmt == "cf32" else 2 * file_dtype.itemsize
    n_file = os.path.getsize(path) // item_bytes
    dev = torch.device("cuda", torch.cuda.current_device())
    # a filter in front hands on whole segments: up to one of them more than a chunk holds
    filt = None if notch is None else pkg.FftFilter(notch)
    room = chunk_items + 4096 + (0 if filt is None else 2048)
    # packets_only: nothing between the Costas loop and the packer is written to memory (the app delivers packets); the
    # symbol tap of --zmq needs SyncwordRemove's output stream, i.e. the full form
    rx = pkg.NativePacketReceiver(4, syncword_freq_bins, syncword_threshold, max_items=room,
                                  tags_cap=chunk_items // 768 + 64, decode_headers=True, packets_only=zmq_ports is None)
    if zmq_ports is not None:  # packet_receiver.hpp:163-168
        rx.publish_symbol_pdus(f"tcp://*:{zmq_ports[0]}", f"tcp://*:{zmq_ports[1]}")
    ddc = None
    if tune is not None or decimate is not None:
        dec, interp = (1, 1) if decimate is None else (decimate if isinstance(decimate, tuple) else decimation(decimate))
        if fft_ddc:
            ddc = pkg.FftDdc([0.0 if tune is None else tune], dec)
        else:
            ddc = pkg.Ddc([0.0 if tune is None else tune], dec, interpolation=interp, max_frames=room - 4096)
    fft = 3072  # smallest batch the receiver takes in this mode (one header window + one FFT block)
    pinned = [torch.empty(shape, dtype=file_dtype).pin_memory() for _ in range(2)]
    staged = [torch.empty(shape, dtype=file_dtype, device=dev) for _ in range(2)]
    work = torch.empty(room, dtype=torch.complex64, device=dev)
    filtered = None if filt is None else torch.empty(chunk_items + 2048, dtype=torch.complex64, device=dev)
    copy_stream = torch.cuda.Stream()
    events = [torch.cuda.Event(), torch.cuda.Event()]
    packets, stats = [], {"headers": 0, "invalid_headers": 0, "crc_failures": 0}
    fh = open(path, "rb")

    def load(slot):
        """file -> pinned -> device (asynchronously on the copy stream); returns items read"""
        view = pinned[slot].numpy().view(np.uint8)
        got = fh.readinto(memoryview(view)) // item_bytes
        if got:
            with torch.cuda.stream(copy_stream):
                staged[slot][:got].copy_(pinned[slot][:got], non_blocking=True)
                events[slot].record(copy_stream)
        return got

    def deliver(res):
        m = res["header_messages"]
        stats["headers"] += int(m.size)
        stats["invalid_headers"] += int(np.sum(m["invalid_header"] != 0))
        lens = res["packet_lengths"]
        stats["crc_failures"] += int(np.sum(lens == 0))
        data = res["packets"].cpu().numpy()
        pos = 0
        for n in lens[lens > 0]:
            n = int(n)
            packets.append(data[pos:pos + n].tobytes())
            pos += n

    t0 = time.perf_counter()
    slot, left, done = 0, 0, 0
    got = load(slot)
    while got or left >= fft:
        nxt = 0
        if got:
            torch.cuda.current_stream().wait_event(events[slot])
            if filt is not None:
                # the notch first: the chunk's whole segments as complex64, and at the end of the file what is still owed
                got = filt.process_bulk(staged[slot][:got], scale=None if fmt == "cf32" else scale, out=filtered).numel()
                nxt = load(slot ^ 1)
                if not nxt:
                    got += filt.flush(out=filtered[got:]).numel()
                if ddc is not None:
                    got = ddc.process_bulk(filtered[:got], out=work[left:left + got].unsqueeze(0)).shape[1] if got else 0
                else:
                    work[left:left + got].copy_(filtered[:got])
            else:
                if ddc is not None:
                    got = ddc.process_bulk(staged[slot][:got], out=work[left:left + got].unsqueeze(0),
                                           scale=None if fmt == "cf32" else scale).shape[1]
                elif fmt == "cf32":
                    work[left:left + got].copy_(staged[slot][:got])
                else:
                    pkg.iq_unpack(staged[slot][:got], scale, out=work[left:left + got])
                nxt = load(slot ^ 1)          # the next chunk travels while this one is processed
        n = left + got
        if n < fft:
            break
        res = rx.process_bulk(work[:n])
        deliver(res)
        c = res["consumed"]
        done += c
        left = n - c
        if left:
            work[:left].copy_(work[c:n].clone())
        slot ^= 1
        got = nxt
        if not got and left < fft:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    fh.close()
    if out:
        with open(out, "wb") as f:
            for p in packets:
                f.write(len(p).to_bytes(2, "big"))
                f.write(p)
    return {"packets": packets, "items": done, "file_items": n_file, "seconds": dt, **stats}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input_file")
    ap.add_argument("syncword_freq_bins", nargs="?", type=int, default=4)   # packet_receiver_file.cpp:25
    ap.add_argument("syncword_threshold", nargs="?", type=float, default=9.5)  # :26
    ap.add_argument("--out", help="write the received packets here (uint16 big-endian length + bytes each)")
    ap.add_argument("--chunk-items", type=int, default=1 << 24)
    ap.add_argument("--zmq", action="store_true", help="publish header / payload symbol PDUs on ZeroMQ PUB sockets (tcp 5000 / 5001)")
    ap.add_argument("--zmq-ports", type=int, nargs=2, metavar=("HEADER", "PAYLOAD"), help="... on these ports instead")
    ap.add_argument("--format", choices=list(FILE_DTYPES), default="cf32", help="the file's items (default: complex64)")
    ap.add_argument("--scale", type=float, help="of an integer format's components (default: 2^-15 for sc16, else 2^-7)")
    ap.add_argument("--tune", type=tune_value, metavar="CYCLES_PER_SAMPLE|auto",
                    help="the carrier's offset in the file (a Ddc in front).  auto: scan the file as --scan does and tune to the "
                         "carrier of greatest power; the value is as good as the scan's resolution of one PSD bin (1/2048), "
                         "which stays inside the detector's pull-in range of 0.00673 / D for --decimate <= 13")
    ap.add_argument("--scan", action="store_true", help="print one line per carrier (frequency, bandwidth, snr_db) and exit")
    ap.add_argument("--scan-items", type=int, metavar="N", help="scan the first N items of the file only (default: all)")
    ap.add_argument("--bursts", action="store_true",
                    help="with --scan: a second pass through a Spectrogram, then one line per burst of every carrier "
                         "(frequency, start and end in file samples, snr_db)")
    ap.add_argument("--waterfall", metavar="FILE.npy", help="with --scan: write the Spectrogram's rows (float32 [rows, 2048], FFT bin order)")
    ap.add_argument("--waterfall-average", type=int, default=1, metavar="R", help="segments per row of --bursts and --waterfall (1 .. 64, default 1)")
    ap.add_argument("--decimate", type=decimation_or_auto, metavar="N[/M]|auto",  # argparse reports a type's ValueError as a usage error
                    help="file samples per receiver sample, an integer or a ratio such as 25/4 (a Ddc in front).  auto: measure "
                         "the tuned carrier's symbol rate on its bursts (LineSpectrum) and take the simplest ratio that puts 4 "
                         "samples on a symbol; needs --tune")
    ap.add_argument("--refine", action="store_true",
                    help="with --tune: add the residual carrier offset a LineSpectrum finds on the carrier's bursts (the line of "
                         "x^4, good to a small fraction of the scan's bin) to the tuned frequency")
    ap.add_argument("--burst-rows", action="store_true",
                    help="with --tune and --decimate (values or auto): extract the carrier's bursts, bring every burst row to 4 "
                         "samples per symbol and remove its residual offset with a RowResampler, each row by its own "
                         "LineSpectrum reading, and receive the rows; no streaming Ddc runs over the file, which has to fit "
                         "one chunk")
    ap.add_argument("--fft-ddc", action="store_true",
                    help="with --tune and a power-of-two --decimate of 4 .. 64: an FftDdc (the fast-convolution form, DESIGN "
                         "section 25) in place of the Ddc; it delivers whole segments, so up to one hop of samples at the "
                         "end of the file stays undelivered")
    ap.add_argument("--notch", action="append", type=notch_band, metavar="F:BW",
                    help="remove the band BW cycles per file sample wide around F from the file's samples before anything else "
                         "sees them (an FftFilter, DESIGN section 32); repeatable")
    ap.add_argument("--notch-taps", type=int, default=1025, metavar="N", help="taps of the --notch design (odd, 3 .. 1985; default 1025)")
    a = ap.parse_args(argv)
    if a.notch and (a.scan or a.tune == "auto" or a.refine or a.decimate == "auto" or a.burst_rows):
        ap.error("--notch goes with none of --scan, --tune auto, --refine, --decimate auto, --burst-rows")
    if a.notch and a.chunk_items < 2048:
        ap.error("--notch needs --chunk-items of at least 2048")
    if a.fft_ddc:
        d = a.decimate
        if (a.tune is None or not isinstance(d, tuple) or d[1] != 1 or d[0] not in (4, 8, 16, 32, 64) or a.burst_rows
                or a.scan):
            ap.error("--fft-ddc needs --tune and --decimate 4, 8, 16, 32 or 64 (no ratio, not auto), and goes with neither "
                     "--burst-rows nor --scan")
    if a.burst_rows and (a.tune is None or a.decimate is None or a.scan or a.zmq or a.zmq_ports):
        ap.error("--burst-rows needs --tune and --decimate (values or auto) and goes with neither --scan nor --zmq")
    if (a.bursts or a.waterfall) and not a.scan:
        ap.error("--bursts and --waterfall belong to --scan")
    blind = a.refine or a.decimate == "auto" or a.burst_rows
    if blind and a.tune is None:
        ap.error("--refine and --decimate auto need --tune (a value or auto)")
    if a.scan or a.tune == "auto" or blind:
        carriers, spectrum, items = scan_file(a.input_file, a.format, a.scale, a.scan_items, a.chunk_items)
        print_carriers(carriers, spectrum, items)
        if a.scan and (a.bursts or a.waterfall):
            sg, power, rows = scan_rows(a.input_file, carriers if a.bursts else carriers[:0], a.format, a.scale, a.scan_items,
                                        a.chunk_items, a.waterfall_average, keep_rows=bool(a.waterfall))
            if a.bursts:
                print_bursts(sg, carriers, power)
            if a.waterfall:
                np.save(a.waterfall, rows)
        if a.scan:
            return
        if not len(carriers):
            sys.exit("--tune auto: the scan found no carrier" if a.tune == "auto" else "--refine / --decimate auto: the scan found no carrier")
        if a.tune == "auto":
            carrier = carriers[int(np.argmax(carriers["power"]))]
            a.tune = float(carrier["frequency"])
            print(f"--tune auto: {a.tune:+.6f}")
        else:  # the carrier the given frequency means: the nearest on the circle
            away = np.abs(carriers["frequency"] - a.tune)
            carrier = carriers[int(np.argmin(np.minimum(away, 1.0 - away)))]
        if a.burst_rows:
            item_bytes = 8 if a.format == "cf32" else 2 * FILE_DTYPES[a.format].itemsize
            if os.path.getsize(a.input_file) // item_bytes > a.chunk_items:
                sys.exit(f"--burst-rows: the file has more than --chunk-items = {a.chunk_items} items")
            b = burst_rows_of_file(a.input_file, a.tune, float(carrier["bandwidth"]), a.format, a.scale, None, a.chunk_items)
            if b["rows"] is not None and b["good"].any():
                d0 = b["decimation"]
                rate = None if a.decimate == "auto" else d0 * a.decimate[1] / (4.0 * a.decimate[0])  # symbols per row item
                r = receive_burst_rows(b, a.syncword_freq_bins, a.syncword_threshold, rate, a.out)
                print(f"--burst-rows: {b['rows'].shape[0]} rows at decimation {d0} ({int(b['good'].sum())} with a carrier line), "
                      f"symbols per file sample {np.round(r['rates'] / d0, 7).tolist()}, offsets "
                      f"{[float(f'{v / d0:+.3e}') for v in r['offsets']]}: resampled row by row, no streaming pass over the file")
                print(f"{r['items']} row samples in {r['seconds']:.3f} s; headers {r['headers']} ({r['invalid_headers']} invalid), "
                      f"packets {len(r['packets'])} ({r['crc_failures']} CRC failures), {sum(len(p) for p in r['packets'])} bytes")
                return
            print("--burst-rows: no burst row shows a carrier line 6 dB above the rest: falling back to the streaming path")
        if a.refine or a.decimate == "auto":
            r = refine_file(a.input_file, a.tune, float(carrier["bandwidth"]), a.format, a.scale, a.scan_items, a.chunk_items)
            if a.refine:
                if r["offset"] is None:
                    sys.exit(f"--refine: none of the {r['rows']} rows at decimation {r['decimation']} shows a line 6 dB above the rest")
                a.tune += r["offset"]
                print(f"--refine: {r['offset']:+.3e} from {r['rows']} rows at decimation {r['decimation']}: --tune {a.tune:+.7f}")
            if a.decimate == "auto":
                if r["rate"] is None:
                    sys.exit(f"--decimate auto: none of the {r['rows']} rows at decimation {r['decimation']} shows a carrier line to read the symbol rate beside")
                interp, dec = ge.load_package().resample_ratio(r["rate"])
                a.decimate = (dec, interp)
                print(f"--decimate auto: {r['rate']:.6f} symbols per file sample: --decimate {dec}/{interp}")
    zmq_ports = tuple(a.zmq_ports) if a.zmq_ports else ((5000, 5001) if a.zmq else None)
    notch = ge.load_package().band_filter_taps(a.notch, "stop", a.notch_taps) if a.notch else None
    r = receive_file(a.input_file, a.syncword_freq_bins, a.syncword_threshold, a.chunk_items, a.out, zmq_ports=zmq_ports,
                     fmt=a.format, scale=a.scale, tune=a.tune, decimate=a.decimate, fft_ddc=a.fft_ddc, notch=notch)
    print(f"{r['items']} of {r['file_items']} samples in {r['seconds']:.3f} s = {r['items'] / r['seconds'] / 1e6:.1f} Msps "
          f"(file and PCIe included); headers {r['headers']} ({r['invalid_headers']} invalid), packets "
          f"{len(r['packets'])} ({r['crc_failures']} CRC failures), {sum(len(p) for p in r['packets'])} bytes")


if __name__ == "__main__":
    main()
