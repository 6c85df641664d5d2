"""The yardsticks of the filter path, restated on the host in the plainest way.

select_bytes is the selector's whole contract in one line; byte_mask gives the same per byte, so that any feed range can be
compared on its own.  decide restates the filter's rule record by record in Python integers, independently of the numpy
form in pykmer_amd.filter.  record_starts_ref cuts a FASTA or FASTQ text into records from the oracle's parse."""
import numpy as np

import oracle
from fastq_ref import fastq_to_fasta, lines


def select_bytes(text: bytes, starts, keep) -> bytes:
    return b"".join(text[int(starts[r]):int(starts[r + 1])] for r in range(len(keep)) if keep[r])


def byte_mask(n_bytes: int, starts, keep) -> np.ndarray:
    """(n_bytes,) bool: byte o lies in a kept record.  Offsets beyond the text are cut at its end."""
    mask = np.zeros(n_bytes, dtype=bool)
    for r in range(len(keep)):
        if keep[r]:
            mask[int(starts[r]):int(starts[r + 1])] = True
    return mask


def records_kept(bytes_fed: int, starts, keep) -> int:
    limit = min(int(bytes_fed), int(starts[-1]))
    return sum(1 for r in range(len(keep)) if keep[r] and int(starts[r]) < limit)


def decide(hits, n_valid, min_hits: int = 1, min_percent: int = 0, min_tables: int = 1):
    """(matched (R,), match (R, N)) as lists of bools, in Python integers: table t matches record r iff hits >= H and
    100 hits >= P n_valid, never without a valid window; the record matches iff at least M tables do."""
    matched, match = [], []
    for r in range(len(n_valid)):
        nv = int(n_valid[r])
        row = [nv > 0 and int(h) >= min_hits and 100 * int(h) >= min_percent * nv for h in hits[r]]
        match.append(row)
        matched.append(sum(row) >= min_tables)
    return matched, match


def record_starts_ref(text: bytes, fmt: str = "fasta") -> np.ndarray:
    """(R + 1,) uint64: the offset of every record's '>' or '@' in `text`, and the length of the text."""
    if fmt == "fastq":
        fastq_to_fasta(text)                                 # raises on a malformed stream, as the device does
        ls, starts = lines(bytes(text)), []
        for r in range(0, len(ls), 4):
            if ls[r][0] == ls[r][1]:                         # an empty line 1: only blank lines follow, and they stay with the last record
                break
            starts.append(ls[r][0])
    else:
        recs = oracle.count_fasta(text, 1)["records"]
        starts = [int(r["name_off"]) - 1 for r in recs]
    return np.array(starts + [len(text)], dtype=np.uint64)

