"""The texts and tables of the mask tests (test_gpu_cover.py, test_gpu_mask.py; test_mask_host.py checks on the CPU what they
rely on).  The texts come from the existing builders (query_coords_inputs, query_ref); the tables are made here so that every
text holds covered and uncovered bases under every count window.  Built once per process; every builder is deterministic."""
import functools

import numpy as np

import oracle
import query_coords_inputs as qci
import query_ref

CHUNK = 16384
WINDOWS = ((1, 255), (2, 254), (255, 255))
KS = (5, 9, 15)
BAND = (0, 0, 1, 2, 254, 0, 255, 17, 0, 3)                  # the count of a band of windows: every window edge, and gaps


class BandTable:
    """A 4^k-byte table known where it is non-zero: keys (sorted k-mers) and vals.  Indexable by k-mers like an array."""

    def __init__(self, k: int, keys, vals):
        self.k, self.keys, self.vals = k, np.asarray(keys, dtype=np.uint64), np.asarray(vals, dtype=np.uint8)

    def __getitem__(self, kmers) -> np.ndarray:
        kmers = np.asarray(kmers, dtype=np.uint64)
        if self.keys.size == 0:
            return np.zeros(kmers.size, dtype=np.uint8)
        at = np.minimum(np.searchsorted(self.keys, kmers), self.keys.size - 1)
        return np.where(self.keys[at] == kmers, self.vals[at], 0).astype(np.uint8)

    def dense(self) -> np.ndarray:
        out = np.zeros(4 ** self.k, dtype=np.uint8)
        out[self.keys.astype(np.int64)] = self.vals
        return out


def texts(k: int):
    """(name, text) of the texts every count window is tried on at k."""
    return [("one_record", qci.one_record()), ("gapped", qci.gapped(k)[0]), ("blanks", qci.blanks()), ("many_127", qci.many_records(127)),
            ("many_200", qci.many_records(200)), ("reads", query_ref.reads_case(k))]


@functools.lru_cache(maxsize=None)
def band_tables(k: int):
    """Two BandTables at k: the valid windows of texts(k), in text order, cut into bands of 23 (31) windows; a band's k-mers
    get the band's count from BAND (the first band that holds a k-mer decides).  Bands of count 0 leave stretches no table
    covers; 1, 2, 254 and 255 are the edges of the count windows."""
    kmers = np.concatenate([oracle.kmer_list(t, k) for _, t in texts(k)])
    out = []
    for width, phase in ((23, 0), (31, 4)):
        band = np.array(BAND, dtype=np.uint8)[(np.arange(kmers.size) // width + phase) % len(BAND)]
        keys, first = np.unique(kmers, return_index=True)
        vals = band[first]
        out.append(BandTable(k, keys[vals != 0], vals[vals != 0]))
    return tuple(out)


# ------------------------------------------------------------------ seams
SEAM_K = 13                                                  # few chance matches: the matching windows are the ones meant


def seam_text() -> bytes:
    return qci.one_record()                                  # 40 000 bases on 60-column lines: three chunks


@functools.lru_cache(maxsize=None)
def seam_tables():
    """(around, edge) for seam_text() at SEAM_K.  around: counted from query_ref.counted_text_for -- the windows within 400
    bases of a 16 KiB boundary match.  edge: per boundary only the window whose first base is the last base in front of the
    boundary: that base lies in no other matching window, and its window ends in the next chunk."""
    text, k = seam_text(), SEAM_K
    around = oracle.count_fasta(query_ref.counted_text_for(text, k, seed=1900), k)["table"]
    start, _, first_base = query_ref.straddling_windows(text, k)
    kmers = oracle.kmer_list(text, k)
    assert start.size == kmers.size
    edge = np.zeros(4 ** k, dtype=np.uint8)
    for b, at in first_base.items():
        i = int(np.searchsorted(start, at - 1))
        assert start[i] == at - 1
        edge[int(kmers[i])] = 1
    return around, edge


def seam_cuts():
    """Feed cuts around the first chunk seam of seam_text(): every byte from SEAM_K + 2 before it to SEAM_K + 2 behind it."""
    return list(range(CHUNK - SEAM_K - 2, CHUNK + SEAM_K + 3))


def line_cuts():
    """One byte at a time over one line: the 62 cuts from a line's first byte to the next line's."""
    head = seam_text().index(b"\n") + 1
    first = head + 61 * 100
    return list(range(first, first + 62))


# ------------------------------------------------------------------ a run across a chunk without k - 1 bases
@functools.lru_cache(maxsize=None)
def hollow():
    """(text, table) at SEAM_K: one record whose middle chunk holds three valid bases and otherwise blank lines and line
    terminators -- none of which breaks the run -- so that windows lie across three slots.  The table is counted from the 40
    bases around the hollow and from a stretch well inside the first chunk."""
    rng = np.random.default_rng(1901)
    k = SEAM_K
    head = b">hollow\n"
    lines_a = (CHUNK - len(head)) // 61
    seq_a = query_ref._bases(rng, 60 * lines_a + (CHUNK - len(head) - 61 * lines_a - 1))
    part_a = head + b"".join(seq_a[i:i + 60] + b"\n" for i in range(0, len(seq_a), 60))
    assert len(part_a) == CHUNK and part_a.endswith(b"\n") and not part_a.endswith(b"\n\n")
    filler = (b"\n", b" \n", b"\r\n", b"\t \r", b"\n\n")
    middle = [b"ACG\n"]
    while sum(map(len, middle)) < CHUNK - 8:
        middle.append(filler[len(middle) % len(filler)])
    middle.append(b"\n" * (CHUNK - sum(map(len, middle))))
    middle = b"".join(middle)
    seq_c = query_ref._bases(rng, 9000)
    text = part_a + middle + b"".join(seq_c[i:i + 60] + b"\n" for i in range(0, len(seq_c), 60))
    assert len(middle) == CHUNK and 2 * CHUNK < len(text) < 3 * CHUNK
    counted = b">across\n" + seq_a[-20:] + b"ACG" + seq_c[:20] + b"\n>inside\n" + seq_a[3000:3100] + b"\n"
    return text, oracle.count_fasta(counted, k)["table"]


# ------------------------------------------------------------------ more chunks than the scan tile
@functools.lru_cache(maxsize=None)
def long_text():
    """(text, table) at SEAM_K: one record of 1026 chunks on 60-column lines; the table holds the k-mers of three stretches of
    it, one of them across the seam of the 1024-chunk scan tile."""
    rng = np.random.default_rng(1902)
    k = SEAM_K
    n = 1026 * CHUNK * 60 // 61 - 100
    seq = query_ref._bases(rng, n)
    text = query_ref._record(b"long", seq)
    assert 1025 * CHUNK < len(text) <= 1026 * CHUNK
    at = 1024 * CHUNK * 60 // 61
    counted = b">a\n" + seq[at - 150:at + 150] + b"\n>b\n" + seq[5000:5200] + b"\n>c\n" + seq[n - 200:] + b"\n"
    return text, oracle.count_fasta(counted, k)["table"]


# ------------------------------------------------------------------ mask.py end to end
DONOR = b"TTGACCAGGTAACGTACGTTAGCACGTGGATCCAATTGGCACTGA"
HOST = b"GATTACAGATTACAGGTACCTTAGGCATCGATCGGATATCCGGA"
# wrapped lines, lower case, CRLF, text before the first header, records without a valid window, no final newline
TOOL_FASTA = (b"ACGTACGTAC dead text\n\n>  donor piece \t\n" + DONOR[:20] + b"\r\n" + DONOR[20:41].lower() + b"\n>none\nNNNNNNNN\n>empty\n>tiny\nACG\n>host piece\n"
              + HOST[3:40] + b"\n>mixed\n" + DONOR[5:25] + b"N" + HOST[8:30] + b"\n>other\nCCCCCCCCCCCCAAAAAAAAAAAATTTT\n>last donor\n" + DONOR[10:])
