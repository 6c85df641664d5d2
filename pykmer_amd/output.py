"""How every tool writes an output file: announced, through `<path>.tmp`, renamed once it is complete."""
import json
import pathlib
from contextlib import contextmanager
from json import JSONEncoder
from pathlib import Path


class _Encoder(JSONEncoder):
    """merger.py:23-30 patches JSONEncoder globally so Path objects serialise as strings; same effect, scoped."""

    def default(self, obj):
        if isinstance(obj, pathlib.PurePath):
            return str(obj)
        if hasattr(obj.__class__, "to_dict"):
            return obj.to_dict()
        return super().default(obj)


@contextmanager
def atomic_write(path, mode: str):
    """Prints `saving <path>`, opens `<path>.tmp` in `mode` for the block and renames it to `path` after a clean exit.  If
    the block raises, `path` does not appear (and the `.tmp` stays behind, half-written)."""
    print(f"saving {path}")
    tmp = Path(f"{path}.tmp")
    with tmp.open(mode=mode) as fhd:
        yield fhd
    tmp.rename(path)


def write_json(path, obj) -> None:
    """`obj` as the tools' metadata JSON (sorted keys, indent 1, Paths as strings, Headers as dicts), through atomic_write."""
    with atomic_write(path, "wt") as fhd:
        json.dump(obj, fhd, sort_keys=True, indent=1, cls=_Encoder)
