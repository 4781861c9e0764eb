"""What --format adds to tools/benchmark_duc.py, benchmark_fft_duc.py and benchmark_fft_duc_mixed.py:
for a shape the tool already measures, three figures from the same process -- the fused call that writes sc16 / sc8 /
cu8 from the kernel, the complex64 call, and the complex64 call followed by iq_pack().  The gain is a quarter of the
format's default on rows of unit normal items, so a component clips beyond 4 sigma of the band.  How many workgroups
then add to the counter depends on the shape: with K = 8 rows summed the band's sigma is above 1 and nearly every tile of
2048 samples clips something; with K = 1 and the default prototype it is about 1, a component clips with probability
6e-5 or less, and about one workgroup in nine issues the atomic (counted).  The fused call is timed with the atomics that such a signal
causes, which is not one per workgroup in every shape."""


def iq_out_figures(pkg, torch, median_ms, iters, fmt, n, call):
    """call(**kw): the shape's process_bulk() with the tool's input, kw = out / format / gain / clipped; returns its
    result.  n: the most samples a call makes.  Returns the JSON fields."""
    dtype = {"sc16": torch.int16, "sc8": torch.int8, "cu8": torch.uint8}[fmt]
    gain = 0.25 * (32768.0 if fmt == "sc16" else 128.0)
    band = torch.empty(n, dtype=torch.complex64, device="cuda")
    iq = torch.empty((n, 2), dtype=dtype, device="cuda")
    clipped = torch.zeros(1, dtype=torch.int64, device="cuda")

    def two_calls():
        x = call(out=band)
        pkg.iq_pack(x, fmt, gain, out=iq[:x.numel()], clipped=clipped)

    ms_fused = median_ms(lambda: call(out=iq, format=fmt, gain=gain, clipped=clipped), iters, torch)
    ms_c64 = median_ms(lambda: call(out=band), iters, torch)
    ms_two = median_ms(two_calls, iters, torch)
    return {"format": fmt, "fused_ms": round(ms_fused, 4), "complex64_ms": round(ms_c64, 4), "two_call_ms": round(ms_two, 4),
            "fused_over_complex64": round(ms_fused / ms_c64, 3), "fused_over_two_call": round(ms_fused / ms_two, 3)}
