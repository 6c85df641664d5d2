"""The list of `.kin[.bgz]` tables a tool is given: its `data` entries (what every output's json says about its inputs) and
the checks the tools share."""
from pathlib import Path
from typing import Sequence

from .header import Header

EXTS = ("." + Header.IND_EXT, "." + Header.IND_EXT + "." + Header.COMP_EXT, ".kma", ".kma." + Header.COMP_EXT)
MAX_KMER_LEN = 17                   # one unsliced 4^k-byte table per sample


def name_of(table) -> str:
    return str(getattr(table, "index_file", None) or getattr(table, "project_name", table))


def description_file(kin) -> Path:
    """The `.kin.json` beside a `.kin` or a `.kin.bgz`."""
    kins = str(kin)
    return Path((kins[:-(len(Header.COMP_EXT) + 1)] if kins.endswith("." + Header.COMP_EXT) else kins) + "." + Header.DESC_EXT)


def table_entry(pos: int, kin, load, **more) -> dict:
    """The `data` entry of table number `pos` of a tool's list: `load(kin)` is the tool's own way to a Header (and to say
    what is wrong with the file).  The header is the Header itself until lean_headers."""
    print(f"verifying {kin}")
    return {"pos": pos, **more, "index_file": Path(kin), "description_file": description_file(kin), "header": load(kin)}


def lean_headers(data: list) -> None:
    """Every entry's Header -> the dict written to the json (merger.py:187-188), once the pass no longer needs the Headers."""
    for v in data:
        v["header"] = v["header"].to_dict(lean=True)


def common_kmer_len(tables: Sequence, tool_name: str, kmer_len_of=lambda t: int(t.kmer_len)) -> int:
    """The kmer_len all `tables` share: positive, odd and at most MAX_KMER_LEN; ValueError naming the table otherwise."""
    kmer_len = None
    for t in tables:
        k = kmer_len_of(t)
        if k < 1 or k % 2 == 0:
            raise ValueError(f"{name_of(t)}: kmer_len {k} is not positive and odd")
        if k > MAX_KMER_LEN:
            raise ValueError(f"{name_of(t)}: kmer_len {k} is beyond the {tool_name} path (at most {MAX_KMER_LEN}: one unsliced table)")
        if kmer_len is None:
            kmer_len = k
        elif k != kmer_len:
            raise ValueError(f"{name_of(t)}: kmer_len {k} differs from the {kmer_len} of {name_of(tables[0])}")
    return kmer_len
