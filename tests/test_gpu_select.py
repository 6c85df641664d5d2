"""GPU: the record selector (kmer_select.hip, pk_select_*) against one line of Python over the raw bytes, cut per feed range:
every feed must hand back exactly the bytes of its own stretch of the stream that lie in kept records.  Exact equality."""
import ctypes

import numpy as np
import pytest

import filter_ref

pytestmark = pytest.mark.gpu

CHUNK = 16384
LENGTHS = (0, 1, 2, 63, 64, 65)
FEEDS = (None, 1, 7, 63, 64, 65, 4097, 16384, 16385)     # None: the stream whole


def _stream(seed: int, n_bytes: int, lead: int = 0, trail: int = 0):
    """(text, starts, keep): records of the edge lengths and of 1-300 bytes, `lead` bytes before the first and `trail`
    behind the last, random flags."""
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < n_bytes - lead - trail:
        lens.append(int(rng.choice(LENGTHS)) if rng.random() < 0.4 else int(rng.integers(1, 301)))
    starts = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    text = rng.integers(0, 256, int(starts[-1]) + trail, dtype=np.uint8)
    keep = rng.integers(0, 2, len(lens), dtype=np.uint8)
    return text, starts, keep


def _check_feeds(gpu, text, starts, keep, feed, want_mask=None):
    """Feeds `text` in pieces of `feed` bytes (None: whole) and compares every piece's output with the reference's."""
    mask = filter_ref.byte_mask(len(text), starts, keep) if want_mask is None else want_mask
    step = len(text) if feed is None else feed
    with gpu.Selector(0) as sel:
        sel.set_records(starts, keep)
        at = 0
        while True:
            piece = text[at:at + step]
            got = sel.feed(piece)
            want = piece[mask[at:at + len(piece)]]
            assert np.array_equal(got, want), (feed, at, got.size, want.size)
            at += len(piece)
            if at >= len(text):
                break
        fin = sel.finish()
    assert fin == {"bytes_fed": len(text), "bytes_kept": int(mask.sum()), "records_kept": filter_ref.records_kept(len(text), starts, keep)}
    return mask


@pytest.fixture(scope="module")
def three_chunks():
    text, starts, keep = _stream(11, 40 * 1024)
    assert 2 * CHUNK < len(text) <= 3 * CHUNK + 400
    mask = filter_ref.byte_mask(len(text), starts, keep)
    assert np.array_equal(text[mask], np.frombuffer(filter_ref.select_bytes(text.tobytes(), starts, keep), dtype=np.uint8))
    return text, starts, keep, mask


@pytest.mark.parametrize("feed", FEEDS)
def test_random_streams_in_feeds_of_every_size(gpu, three_chunks, feed):
    """The three-chunk stream whole and in feeds of every size; the feeds of 1 and 7 bytes, each a launch of its own that
    never sees a second chunk, run over a stream of 5 KiB instead (thousands of feeds, not tens of thousands)."""
    text, starts, keep, mask = three_chunks
    if feed in (1, 7):
        text, starts, keep = _stream(12, 5 * 1024, lead=3, trail=2)
        mask = None
    _check_feeds(gpu, text, starts, keep, feed, mask)


@pytest.mark.parametrize("seed,n_bytes,lead,trail", [(1, 5000, 0, 0), (2, 20000, 37, 129), (3, 33000, 16384, 1), (4, 700, 3, 16500)])
def test_text_outside_the_records_is_never_emitted(gpu, seed, n_bytes, lead, trail):
    """starts[0] > 0 and starts[R] below the stream length: the binary search's bounds."""
    text, starts, keep = _stream(seed, n_bytes, lead, trail)
    for feed in (None, 65, 16385):
        _check_feeds(gpu, text, starts, np.ones_like(keep), feed)
        _check_feeds(gpu, text, starts, keep, feed)


@pytest.mark.parametrize("kept", [1, 0])
def test_one_record_across_chunks_and_feeds(gpu, kept):
    """One record of more than two chunks between two short ones, fed in four pieces."""
    rng = np.random.default_rng(5)
    starts = np.array([0, 100, 100 + 2 * CHUNK + 777, 100 + 2 * CHUNK + 900], dtype=np.uint64)
    text = rng.integers(0, 256, int(starts[-1]), dtype=np.uint8)
    _check_feeds(gpu, text, starts, np.array([1 - kept, kept, 1 - kept], dtype=np.uint8), 9000)


def test_many_records_in_one_piece(gpu):
    """32 two-byte records in one 64-byte piece, alternating flags; and the same behind 5 bytes of a dropped record."""
    text = np.arange(200, dtype=np.uint8)
    for first in (0, 5, 64, 67):
        starts = np.concatenate([[0] if first else [], first + 2 * np.arange(33)]).astype(np.uint64)
        keep = np.array(([0] if first else []) + [1, 0] * 16, dtype=np.uint8)
        _check_feeds(gpu, text, starts, keep, None)
        _check_feeds(gpu, text, starts, 1 - keep, 7)


def test_empty_records(gpu):
    """Runs of equal offsets: empty records kept and dropped move no byte, and count as records."""
    text = np.arange(100, dtype=np.uint8)
    starts = np.array([10, 10, 10, 20, 20, 50, 90, 90], dtype=np.uint64)
    for keep in ([1, 1, 1, 0, 1, 0, 1], [0, 0, 0, 1, 0, 1, 0], [1, 0, 1, 1, 1, 1, 1]):
        _check_feeds(gpu, text, starts, np.array(keep, dtype=np.uint8), None)
        _check_feeds(gpu, text, starts, np.array(keep, dtype=np.uint8), 10)


def test_keep_all_keep_none_and_no_records(gpu, three_chunks):
    text, starts, keep, _ = three_chunks
    mask = _check_feeds(gpu, text, starts, np.ones_like(keep), 16385)
    assert mask[int(starts[0]):int(starts[-1])].all()
    _check_feeds(gpu, text, starts, np.zeros_like(keep), 4097)
    with gpu.Selector(0) as sel:
        sel.set_records(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint8))
        assert sel.feed(text[:20000]).size == 0 and sel.feed(b"").size == 0
        assert sel.finish() == {"bytes_fed": 20000, "bytes_kept": 0, "records_kept": 0}
    with gpu.Selector(0) as sel:                             # no records and no offsets at all
        assert gpu.load().pk_select_set_records(sel._h, None, None, 0) == gpu.PK_OK
        assert sel.feed(text[:100]).size == 0


def test_empty_feeds_between_others(gpu, three_chunks):
    text, starts, keep, mask = three_chunks
    with gpu.Selector(0) as sel:
        sel.set_records(starts, keep)
        assert sel.feed(b"").size == 0
        a = sel.feed(text[:20001])
        assert sel.feed(np.zeros(0, dtype=np.uint8)).size == 0
        b = sel.feed(text[20001:])
        assert sel.feed(b"").size == 0
        assert np.array_equal(np.concatenate([a, b]), text[mask])
        assert sel.finish()["bytes_fed"] == len(text)


def _tiled(period_text, period_starts, period_keep, n_tiles, extra):
    """`n_tiles` copies of a small stream back to back plus `extra` bytes of the next copy, as one stream."""
    P = len(period_text)
    text = np.concatenate([np.tile(period_text, n_tiles), period_text[:extra]])
    starts = np.concatenate([np.uint64(P * i) + period_starts[:-1] for i in range(n_tiles)] + [[np.uint64(P * n_tiles)]]).astype(np.uint64)
    keep = np.tile(period_keep, n_tiles)
    return text, starts, keep


@pytest.mark.parametrize("n_bytes", [1024 * CHUNK + 5, (64 << 20) + CHUNK + 5])
def test_one_feed_past_the_scan_step_and_past_the_piece(gpu, n_bytes):
    """One feed just past the 1024 chunks one step of the chunk scan covers, and one just past the 64 MiB piece the library
    cuts a feed into; tiled from a small text so that the reference is a tiled mask."""
    ptext, pstarts, pkeep = _stream(21, 4093)
    ptext = ptext[:int(pstarts[-1])]
    P = len(ptext)
    text, starts, keep = _tiled(ptext, pstarts, pkeep, n_bytes // P, n_bytes % P)
    pmask = filter_ref.byte_mask(P, pstarts, pkeep)
    mask = np.concatenate([np.tile(pmask, n_bytes // P), np.zeros(n_bytes % P, dtype=bool)])
    with gpu.Selector(0) as sel:
        sel.set_records(starts, keep)
        got = sel.feed(text)
        assert np.array_equal(got, text[mask])
        assert sel.finish()["bytes_kept"] == int(mask.sum())


def test_output_one_byte_short(gpu, three_chunks):
    text, starts, keep, mask = three_chunks
    cut = 20000
    need = int(mask[:cut].sum())
    with gpu.Selector(0) as sel:
        sel.set_records(starts, keep)
        out = np.full(need - 1, 0xA5, dtype=np.uint8)
        with pytest.raises(gpu.PkError) as err:
            sel.feed(text[:cut], out=out)
        assert err.value.code == gpu.PK_ERR_RECS_CAP and err.value.needed == need
        assert (out == 0xA5).all()                           # untouched
        out = np.full(need, 0xA5, dtype=np.uint8)
        assert np.array_equal(sel.feed(text[:cut], out=out), text[:cut][mask[:cut]])   # the same feed, with room
        assert np.array_equal(sel.feed(text[cut:]), text[cut:][mask[cut:]])            # and the stream goes on where it was
        assert sel.finish()["bytes_kept"] == int(mask.sum())


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_device_form_into_any_alignment(gpu, three_chunks, shift):
    text, starts, keep, mask = three_chunks
    n = len(text)
    src, dst = gpu.DeviceBuffer(n, 0), gpu.DeviceBuffer(n + 8, 0)
    try:
        src.upload(text)
        dst.upload(np.full(n + 8, 0x5A, dtype=np.uint8))
        with gpu.Selector(0) as sel:
            sel.set_records(starts, keep)
            cut = 16384 + 4096                               # the second feed starts 16-byte aligned in the buffer
            k1 = sel.feed_device(src.ptr, cut, dst.ptr + shift, n)
            k2 = sel.feed_device(src.ptr + cut, n - cut, dst.ptr + shift + k1, n - k1)
            with pytest.raises(ValueError):
                sel.feed_device(src.ptr + 4, 16, dst.ptr, 16)                 # text not 16-byte aligned
            assert sel.timings()["select_s"] > 0 and sel.timings()["feeds"] == 2
        got = dst.download()
        assert k1 == int(mask[:cut].sum()) and k1 + k2 == int(mask.sum())
        assert np.array_equal(got[shift:shift + k1 + k2], text[mask])
        assert (got[:shift] == 0x5A).all() and (got[shift + k1 + k2:] == 0x5A).all()   # not a byte outside the range
    finally:
        src.free()
        dst.free()


def test_device_form_refuses_an_output_inside_the_text(gpu, three_chunks):
    text, starts, keep, _ = three_chunks
    buf = gpu.DeviceBuffer(len(text), 0)
    try:
        buf.upload(text)
        with gpu.Selector(0) as sel:
            sel.set_records(starts, np.ones_like(keep))
            with pytest.raises(ValueError, match="overlaps"):
                sel.feed_device(buf.ptr, 4096, buf.ptr + 100, 4096)
    finally:
        buf.free()


def test_calls_out_of_order(gpu, three_chunks):
    text, starts, keep, _ = three_chunks
    lib = gpu.load()
    n_out = ctypes.c_uint64(0)
    out = np.zeros(64, dtype=np.uint8)
    with gpu.Selector(0) as sel:
        assert lib.pk_select_feed(sel._h, text.ctypes.data, 64, out.ctypes.data, 64, ctypes.byref(n_out)) == gpu.PK_ERR_STATE   # no records yet
        assert lib.pk_select_finish(sel._h, np.zeros(3, dtype=np.uint64).ctypes.data) == gpu.PK_ERR_STATE
        sel.set_records(starts, keep)
        sel.set_records(starts, keep)                        # again before a feed: allowed
        sel.feed(text[:64])
        with pytest.raises(gpu.PkError) as err:
            sel.set_records(starts, keep)
        assert err.value.code == gpu.PK_ERR_STATE
        sel.finish()
        with pytest.raises(gpu.PkError) as err:
            sel.feed(text[64:128])
        assert err.value.code == gpu.PK_ERR_STATE


def test_records_kept_counts_what_was_fed(gpu):
    """The third total: kept records whose first byte lies below min(bytes fed, starts[R]), each once."""
    text = np.arange(120, dtype=np.uint8)
    starts = np.array([10, 30, 30, 60, 100], dtype=np.uint64)
    keep = np.array([1, 1, 0, 1], dtype=np.uint8)
    for fed, want in ((5, 0), (10, 0), (11, 1), (30, 1), (31, 2), (61, 3), (120, 3)):
        with gpu.Selector(0) as sel:
            sel.set_records(starts, keep)
            sel.feed(text[:fed])
            assert sel.finish()["records_kept"] == want == filter_ref.records_kept(fed, starts, keep), fed
