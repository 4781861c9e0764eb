"""What the GPU tests of the front-end blocks share (test_channelizer.py, test_ddc.py, test_duc.py): the package, arrays
to the device and back, bit patterns, a receiver's packets, and the Ddc's and the Duc's frequency pool and random
prototype."""
import numpy as np
import pytest

import _ddc_ref as dref

# 0, exactly 0.5, a negative one, a word with only low bits set; a shape with K channels takes K from its own offset on
FREQ_POOL = [0.0, 0.5, -0.3137, 3.0 * 2.0 ** -32, 0.123456789, -0.05, 0.41, 1.0 / 3.0, -0.4999, 0.25, 0.02, -0.17,
             0.3, -0.26, 0.07, 0.45]


def load_package():
    """the body of a test module's `pkg` fixture"""
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as ge
    return ge.load_package()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def random_taps(D, L, seed=0):
    """a low-pass shape with random signs mixed in: every tap matters, none is tiny"""
    rng = np.random.default_rng(seed)
    return (dref.kaiser_taps64(D, L) * D + 0.05 * rng.standard_normal(L)).astype(np.float32)


def received_packets(r):
    data, lens = r["packets"].cpu().numpy(), r["packet_lengths"]
    got, pos = [], 0
    for n in lens[lens > 0]:
        got.append(data[pos:pos + int(n)].tobytes())
        pos += int(n)
    return got


def exact_iq_forms(n, seed):
    """a complex64 stream of n samples and, as (array, scale) in the order complex64, sc16, sc8, cu8, the forms of it that
    process_bulk() takes: components (u - 127.5) / 128 for bytes u in [64, 192), that is odd multiples of 2^-8 below 1 / 2.
    cu8 unpacks to them at its default scale, sc8 holds 2 u - 255 for a scale of 2^-8 and sc16 64 times that for 2^-14:
    powers of two, so every unpack is exact."""
    u = np.random.default_rng(seed).integers(64, 192, (n, 2))
    x = np.ascontiguousarray(((u - 127.5) / 128.0).astype(np.float32)).view(np.complex64).reshape(n)
    odd = 2 * u - 255
    return x, [(x, None), ((64 * odd).astype(np.int16), 2.0 ** -14), (odd.astype(np.int8), 2.0 ** -8), (u.astype(np.uint8), None)]


def short_calls_of_mixed_formats(pkg, block, x, forms, cycle=(1, 2, 7, 3, 64, 1)):
    """x through `block` in calls of the cycle's lengths, call i in form i mod 4; the rows joined, on the host"""
    import torch
    devs = [(dev(v), s) for v, s in forms]
    for v, s in devs[1:]:
        assert np.array_equal(bits(host(pkg.iq_unpack(v, scale=s))), bits(x))
    parts, lo, i = [], 0, 0
    while lo < x.size:
        hi = min(lo + cycle[i % len(cycle)], x.size)
        v, s = devs[i % 4]
        parts.append(block.process_bulk(v[lo:hi], scale=s))
        lo, i = hi, i + 1
    return host(torch.cat(parts, dim=1))
