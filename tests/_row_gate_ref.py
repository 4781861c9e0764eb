"""A statement of the RowBurstGate's definition (include/gr4pm_hip.h) in NumPy, for the tests.

block_sums(x, B): the block powers of a whole row, bit for bit: per item fl32(fl32(re re) + fl32(im im)); W = min(B, 64)
lane sums t[l] over the block's items l, l + W, ... in ascending order, then folds t[l] += t[l + offset] for offset = W / 2
.. 1.  gate(sums, n_items, ...): the state machine over ALL block sums of a row at once, followed by the flush: the list
of records (dicts).  Row: the same as a stream (process(new items) / flush()), which keeps every item it was given; the
records of a cutting and the burst rows come from it."""
import numpy as np

TRUNCATED, AT_END = 1, 2


def item_power(x):
    x = np.asarray(x, dtype=np.complex64)
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    return (re * re).astype(np.float32) + (im * im).astype(np.float32)  # float32 arrays: every operation rounds once


def block_sums(x, B, pad=False):
    """the sums of the complete blocks of x (pad: a trailing incomplete block too, completed with +0)"""
    p = item_power(x)
    if pad and p.size % B:
        p = np.concatenate([p, np.zeros(B - p.size % B, np.float32)])
    n = p.size // B
    W = min(B, 64)
    p = p[:n * B].reshape(n, B // W, W)
    t = p[:, 0, :].copy()
    for u in range(1, B // W):
        t = t + p[:, u, :]
    off = W // 2
    while off:
        t = t[:, :off] + t[:, off:2 * off]
        off //= 2
    assert t.dtype == np.float32
    return t[:, 0]


def gate(sums, n_items, B, open_sum, close_sum, hold=3, min_blocks=2, pre=4, post=4, max_blocks=64, flush=True):
    """the records of a row whose complete blocks, and with flush the zero-completed trailing one, have these sums.
    open_sum / close_sum: floats, or arrays with one value per block (set_thresholds between calls).
    Returns (records, dropped)."""
    sums = np.asarray(sums, dtype=np.float32)
    nb = sums.size
    opens = np.broadcast_to(np.asarray(open_sum, dtype=np.float32), (nb,))
    closes = np.broadcast_to(np.asarray(close_sum, dtype=np.float32), (nb,))
    out, dropped = [], 0
    b = 0
    while b < nb:
        if not sums[b] >= opens[b]:
            b += 1
            continue
        fa = la = b
        start = max(0, b - pre)
        c, run, end, flags = b, 0, None, 0
        while True:
            if c > fa:
                if sums[c] >= closes[c]:
                    la, run = c, 0
                else:
                    run += 1
                    if run == hold + 1:
                        end = la + post
                        break
            if c - start + 1 == max_blocks:
                end, flags = c, TRUNCATED
                break
            c += 1
            if c == nb:
                break
        if end is None:  # the row ended with the burst open
            if not flush:
                break
            end, flags = min(la + post, nb - 1), AT_END
        if flags != TRUNCATED and la - fa + 1 < min_blocks:
            dropped += 1
        else:
            active = [i for i in range(fa, la + 1) if i == fa or sums[i] >= closes[i]]
            acc = 0.0
            for i in active:
                acc += float(sums[i])
            first, last = start * B, min((end + 1) * B, n_items)
            active_items = min((la + 1) * B, n_items) - fa * B
            out.append(dict(first_item=first, n_items=last - first, first_active_item=fa * B, active_items=active_items,
                            flags=flags, peak=np.float32(max(sums[i] for i in active)), power=acc / active_items))
        b = c + 1
    return out, dropped


class Row:
    """one row as a stream: every item is kept, the records come from gate() over what has been decided so far"""

    def __init__(self, B, open_sum, close_sum, **kw):
        self.B, self.open_sum, self.close_sum, self.kw = B, np.float32(open_sum), np.float32(close_sum), kw
        self.restart()

    def restart(self):
        self.x = np.zeros(0, np.complex64)
        self.opens, self.closes = np.zeros(0, np.float32), np.zeros(0, np.float32)
        self.seen = 0

    def set_thresholds(self, open_sum, close_sum):
        self.open_sum, self.close_sum = np.float32(open_sum), np.float32(close_sum)

    def _run(self, flush):
        sums = block_sums(self.x, self.B, pad=flush)
        more = sums.size - self.opens.size  # these blocks are decided against the current thresholds
        self.opens = np.concatenate([self.opens, np.full(more, self.open_sum, np.float32)])
        self.closes = np.concatenate([self.closes, np.full(more, self.close_sum, np.float32)])
        rec, dropped = gate(sums, self.x.size, self.B, self.opens, self.closes, flush=flush, **self.kw)
        new = rec[self.seen:]
        self.seen = len(rec)
        return new, dropped

    def rows_of(self, records, n_cols):
        out = np.zeros((len(records), n_cols), np.complex64)
        for i, r in enumerate(records):
            out[i, :r["n_items"]] = self.x[r["first_item"]:r["first_item"] + r["n_items"]]
        return out

    def process(self, new):
        """the next items: (the records this call emits, the dropped count so far)"""
        self.x = np.concatenate([self.x, np.asarray(new, dtype=np.complex64)])
        return self._run(False)

    def flush(self, n_cols=None):
        """(records, dropped, their burst rows if n_cols is given); then the created state"""
        rec, dropped = self._run(True)
        rows = self.rows_of(rec, n_cols) if n_cols is not None else None
        self.restart()
        return rec, dropped, rows
