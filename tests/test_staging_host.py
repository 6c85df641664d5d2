"""CPU: the shared host pieces of the table tools -- staging (budget, cuts, the upload loop and who frees what), the output
writer and the table-list checks.  No call here touches a GPU: _lib.DeviceBuffer is a recording fake, the tables are stubs
that log what is read from them, and _lib.mem_info must not be called (every budget is passed or set in the environment)."""
import json
import types

import numpy as np
import pytest

from pykmer_amd import _lib, extract, merger, output, query, staging, tables as table_list


class _FakeBuffer:
    """_lib.DeviceBuffer's shape; every instance is kept in `made`, in allocation order."""
    made = []

    def __init__(self, n_bytes, device=0):
        self.n, self.device, self.ptr = int(n_bytes), device, 0x10000 * (len(_FakeBuffer.made) + 1)
        self.uploads, self.zeroed, self.freed = [], False, 0
        _FakeBuffer.made.append(self)

    def zero(self):
        self.zeroed = True

    def upload(self, data, offset=0):
        assert not self.freed and offset + len(data) <= self.n
        self.uploads.append(len(data))

    def download(self, n_bytes=None, offset=0):
        assert not self.freed
        return np.zeros(self.n if n_bytes is None else n_bytes, dtype=np.uint8)

    def free(self):
        self.freed += 1


class _Table:
    """A file-backed table's shape: data_size and read_table_slice, which logs its ranges (and fails on call `fail_at`)."""

    def __init__(self, data_size, fail_at=None, kmer_len=None):
        self.data_size, self.reads, self.fail_at, self.kmer_len = data_size, [], fail_at, kmer_len

    def read_table_slice(self, lo, hi, threads=1):
        assert threads >= 1
        self.reads.append((lo, hi))
        if len(self.reads) == self.fail_at:
            raise OSError("read failed")
        return np.zeros(hi - lo, dtype=np.uint8)


@pytest.fixture
def device(monkeypatch):
    """The fake in _lib.DeviceBuffer's place; no budget in the environment, and nobody may ask for the free HBM."""
    def no_mem_info(*a):
        raise AssertionError("mem_info called: a budget was neither passed nor set")
    _FakeBuffer.made = []
    monkeypatch.setattr(_lib, "DeviceBuffer", _FakeBuffer)
    monkeypatch.setattr(_lib, "mem_info", no_mem_info)
    monkeypatch.delenv("PK_MERGE_HBM_BUDGET", raising=False)
    return _FakeBuffer


def _formula(lo, hi, n_tables, budget, reserve):
    per_table = max(2048, ((budget - reserve) // n_tables - 64) & ~2047)
    return [(a, min(hi, a + per_table)) for a in range(lo, hi, per_table)]


# ------------------------------------------------------------------ cuts --------------------------
@pytest.mark.parametrize("lo,hi,n_tables,budget,reserve", [
    (0, 4 ** 9, 5, 5 * (40_000 + 64), 0),                    # 38 912 per table: 7 cuts, the last one short
    (4 ** 9 // 2, 4 ** 9, 5, 5 * (40_000 + 64), 0),          # a rank's upper half
    (0, 4 ** 9, 13, 13 * 4096, 0),                           # (4096 - 64) & ~2047 = 2048
    (0, 4 ** 9, 13, 1, 0),                                   # far too small: the floor of 2048
    (0, 4 ** 9, 3, 100_000, 200_000),                        # the reserve exceeds the budget: the floor again
    (64, 10_000, 2, 2 * (4096 + 64), 0),                     # hi - lo no multiple of the cut, lo not 0
    (0, 4 ** 7, 3, 1 << 30, 1 << 20),                        # everything fits: one cut
    (0, 4 ** 9, 18, 1_000_000, 30_000),
])
def test_cuts_are_the_formula_and_tile_the_range(device, lo, hi, n_tables, budget, reserve):
    cuts = staging.sub_slices(lo, hi, n_tables, 0, reserve=reserve, budget=budget)
    assert cuts == _formula(lo, hi, n_tables, budget, reserve)
    assert cuts[0][0] == lo and cuts[-1][1] == hi
    assert all(a < b for a, b in cuts) and all(cuts[i][1] == cuts[i + 1][0] for i in range(len(cuts) - 1))
    assert merger._sub_slices is staging.sub_slices and merger.ResidentTable is staging.ResidentTable


def test_cut_cases_cover_the_floor_and_a_ragged_tail():
    assert _formula(0, 4 ** 9, 13, 1, 0)[0] == (0, 2048) and len(_formula(0, 4 ** 9, 13, 1, 0)) == 128
    ragged = _formula(64, 10_000, 2, 2 * (4096 + 64), 0)
    assert len(ragged) == 3 and ragged[-1][1] - ragged[-1][0] not in (0, 4096)


# ------------------------------------------------------------------ reads, allocation, freeing ----
def _pass(tabs, lo, hi, accumulate=None, **kw):
    """One _flat_partial pass of 4 words over `tabs` (a pass takes its budget from the environment); returns the flat
    accumulator and the (ptrs, n, acc_ptr) of every accumulate call."""
    calls = []

    def default(ptrs, n, acc, device):
        calls.append((list(ptrs), n, acc))
        return 0.25
    flat = merger._flat_partial(tabs, lo, hi, 0, 2, 4, accumulate or default, len(tabs), False, **kw)
    return flat, calls


def test_reads_equal_the_cuts_and_buffers_are_allocated_once(device, monkeypatch):
    N, budget = 5, 5 * (40_000 + 64)
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(budget))
    tabs = [_Table(4 ** 9) for _ in range(N)]
    stats = {}
    flat, calls = _pass(tabs, 0, 4 ** 9, stats=stats)
    cuts = _formula(0, 4 ** 9, N, budget, 0)
    assert len(cuts) == 7 and all(t.reads == cuts for t in tabs)                  # each cut once, in order
    own, bufs = device.made[0], device.made[1:]
    assert own.n == 4 * 8 and own.zeroed and len(bufs) == N                       # the accumulator first, then N slice buffers
    assert all(b.n == max(b_ - a for a, b_ in cuts) for b in bufs)
    assert all(b.uploads == [b_ - a for a, b_ in cuts] for b in bufs)             # refilled per piece, never reallocated
    assert [c[1] for c in calls] == [b_ - a for a, b_ in cuts]
    assert all(c[0] == [b.ptr for b in bufs] and c[2] == own.ptr for c in calls)
    assert flat.dtype == np.uint64 and flat.shape == (4,) and stats["kernel_seconds"] == 0.25 * len(cuts)
    assert all(b.freed == 1 for b in device.made)


def test_buffers_are_freed_when_the_consumer_stops_early(device):
    tabs = [_Table(4 ** 7) for _ in range(3)]
    cuts = staging.sub_slices(0, 4 ** 7, 3, 0, budget=3 * (4096 + 64))
    assert len(cuts) == 4
    pieces = staging.staged_pieces(tabs, cuts, 0, 2)
    assert device.made == []                                                       # nothing before the first piece is asked for
    ptrs, a, b = next(pieces)
    assert (a, b) == cuts[0] and ptrs == [buf.ptr for buf in device.made] and len(device.made) == 3
    assert not any(buf.freed for buf in device.made)
    pieces.close()
    assert all(buf.freed == 1 for buf in device.made) and all(t.reads == cuts[:1] for t in tabs)


def test_buffers_and_accumulator_are_freed_when_a_read_raises(device, monkeypatch):
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(3 * (4096 + 64)))
    tabs = [_Table(4 ** 7), _Table(4 ** 7, fail_at=2), _Table(4 ** 7)]
    with pytest.raises(OSError, match="read failed"):
        _pass(tabs, 0, 4 ** 7)
    assert len(device.made) == 4 and all(b.freed == 1 for b in device.made)
    assert tabs[1].reads == [(0, 4096), (4096, 8192)]


def test_buffers_and_accumulator_are_freed_when_accumulate_raises(device, monkeypatch):
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(3 * (4096 + 64)))
    tabs = [_Table(4 ** 7) for _ in range(3)]

    def failing(ptrs, n, acc, device):
        raise RuntimeError("kernel failed")
    with pytest.raises(RuntimeError, match="kernel failed"):
        _pass(tabs, 0, 4 ** 7, accumulate=failing)
    assert len(device.made) == 4 and all(b.freed == 1 for b in device.made)       # while the exception is still held
    assert all(t.reads == [(0, 4096)] for t in tabs)


def test_a_failed_allocation_frees_the_buffers_before_it(device, monkeypatch):
    class Third(_FakeBuffer):
        def __init__(self, n_bytes, device=0):
            if len(_FakeBuffer.made) == 2:
                raise MemoryError("out of HBM")
            super().__init__(n_bytes, device)
    monkeypatch.setattr(_lib, "DeviceBuffer", Third)
    with pytest.raises(MemoryError):
        next(staging.staged_pieces([_Table(64) for _ in range(4)], [(0, 64)], 0, 2))
    assert len(device.made) == 2 and all(b.freed == 1 for b in device.made)


# ------------------------------------------------------------------ resident tables ---------------
def test_resident_tables_are_one_piece_where_they_lie(device):
    res = [staging.ResidentTable(4096 * (i + 1), 1024, 4 ** 7, first=512) for i in range(3)]
    flat, calls = _pass(res, 640, 1536)                                     # no budget anywhere: nothing has to fit
    assert calls == [([4096 * (i + 1) + (640 - 512) for i in range(3)], 1536 - 640, device.made[0].ptr)]
    assert len(device.made) == 1 and device.made[0].freed == 1                    # the accumulator alone
    assert list(staging.staged_pieces(res, [(512, 1536)], 0, 2)) == [([4096, 8192, 12288], 512, 1536)] and len(device.made) == 1
    with pytest.raises(AssertionError, match="outside the resident part"):
        list(staging.staged_pieces(res, [(0, 4 ** 7)], 0, 2))
    mixed = res[:2] + [_Table(4 ** 7)]
    with pytest.raises(AssertionError, match="cannot be mixed"):
        next(staging.staged_pieces(mixed, [(512, 1536)], 0, 2))
    with pytest.raises(AssertionError, match="cannot be mixed"):
        _pass(mixed, 512, 1536)
    with pytest.raises(AssertionError, match="cannot be mixed"):
        query.stage_tables(mixed, 0)
    assert len(device.made) == 1


# ------------------------------------------------------------------ the budget rule of every pass -
def _record(monkeypatch, name):
    calls = []
    monkeypatch.setattr(_lib, name, lambda ptrs, n, acc, *a, **kw: calls.append(n) or 0.0)
    return calls


def test_occgram_beyond_16_tables_cuts_as_for_one_more(device, monkeypatch):
    N, budget = 17, 2_000_000
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(budget))
    calls = _record(monkeypatch, "occgram_device_accumulate")
    for n_tables, staged in ((17, 18), (16, 16)):
        device.made.clear()
        tabs = [_Table(4 ** 9) for _ in range(n_tables)]
        flat = merger.occgram_partial(tabs, 0, 4 ** 9, 0, 4)
        words = _lib.occgram_words(n_tables)
        cuts = _formula(0, 4 ** 9, staged, budget, words * 8)
        assert len(cuts) == 3 and (staged == n_tables or cuts != _formula(0, 4 ** 9, n_tables, budget, words * 8))
        assert all(t.reads == cuts for t in tabs) and flat.shape == (words,)
        assert device.made[0].n == words * 8 and len(device.made) == 1 + n_tables and all(b.freed == 1 for b in device.made)
    assert len(calls) == 3 + 3


def test_spectrum_reserves_its_own_accumulator_and_the_pair_tally_nothing(device, monkeypatch):
    N = 3
    reserve = _lib.spectrum_words(N) * 8
    budget = reserve + N * (4096 + 64)
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(budget))
    _record(monkeypatch, "spectrum_device_accumulate")
    _record(monkeypatch, "gram_device_accumulate_windows")
    tabs = [_Table(4 ** 7) for _ in range(N)]
    flat = merger.spectrum_partial(tabs, 0, 4 ** 7, 0, 2)
    assert flat.shape == (_lib.spectrum_words(N),) and device.made[0].n == reserve
    assert all(t.reads == _formula(0, 4 ** 7, N, budget, reserve) for t in tabs) and len(tabs[0].reads) == 4

    device.made.clear()
    tabs = [_Table(4 ** 7) for _ in range(N)]                                     # acc_ptr given: nothing reserved, nothing returned
    assert merger.spectrum_partial(tabs, 0, 4 ** 7, 0, 2, acc_ptr=0x7000) is None
    assert all(t.reads == _formula(0, 4 ** 7, N, budget, 0) for t in tabs) and len(tabs[0].reads) == 1
    assert len(device.made) == N and all(b.freed == 1 for b in device.made)

    device.made.clear()
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(N * (4096 + 64)))
    tabs = [_Table(4 ** 7) for _ in range(N)]                                     # the pair tally's accumulator is not budgeted
    parts = merger.gpu_partial(tabs, 0, 4 ** 7, [(1, 255), (2, 9)], 0, 2)
    assert len(parts) == 2 and parts[0].shape == (N, N) and device.made[0].n == 2 * N * N * 8
    assert all(t.reads == _formula(0, 4 ** 7, N, N * (4096 + 64), 0) for t in tabs) and len(tabs[0].reads) == 4


# ------------------------------------------------------------------ query groups ------------------
def test_query_stages_a_group_as_one_whole_piece(device):
    N = 4
    tabs = [_Table(4 ** 7) for _ in range(N)]
    staged = query.stage_tables(tabs, 0, threads=3)
    assert all(t.reads == [(0, 4 ** 7)] for t in tabs)
    assert len(device.made) == N and staged.ptrs == [b.ptr for b in device.made]
    assert all(b.n == 4 ** 7 and b.uploads == [4 ** 7] and not b.freed for b in device.made)
    staged.free()
    staged.free()                                                                  # a second free is harmless
    assert all(b.freed == 1 for b in device.made)

    device.made.clear()
    tabs = [_Table(4 ** 7, fail_at=1 if i == 3 else None) for i in range(N)]
    with pytest.raises(OSError, match="read failed"):
        query.stage_tables(tabs, 0, threads=1)
    assert len(device.made) == N and all(b.freed == 1 for b in device.made)


# ------------------------------------------------------------------ the budget's precedence -------
def test_env_budget_is_honoured_by_every_tool_and_an_explicit_one_wins(device, monkeypatch):
    k, N = 7, 4
    env, explicit = 2 * 4 ** k + 100, 8 * (2048 + 64) * 8
    monkeypatch.setenv("PK_MERGE_HBM_BUDGET", str(env))
    assert staging.hbm_budget(0) == env and staging.hbm_budget(0, 12345) == 12345
    assert staging.hbm_budget(0, workspace=1 << 40) == env and staging.hbm_budget(0, 12345, workspace=1 << 40) == 12345
    # merger: the cuts of a pass
    tabs = [_Table(4 ** k) for _ in range(N)]
    _pass(tabs, 0, 4 ** k)
    assert tabs[0].reads == _formula(0, 4 ** k, N, env, 0) and len(tabs[0].reads) == 3
    # query: the table groups
    def run(query_file, kmer_len, ptrs, mn, mx, dev, first):
        z = np.zeros((1, len(ptrs)), dtype=np.uint64)
        return {"names": ["r"], "seq_len": z[:, 0], "n_valid": z[:, 0], "hits": z, "depth": z}
    qt = [_Table(4 ** k, kmer_len=k) for _ in range(N)]
    assert query.query_records("q.fa", qt, run=run)["n_groups"] == 2
    assert query.query_records("q.fa", qt, run=run, hbm_budget=4 ** k)["n_groups"] == 4
    assert all(t.reads == [(0, 4 ** k)] * 2 for t in qt)
    # extract: 7 / 8 of the budget for the slices
    def call(ptrs, off, n, first_addr, cap):
        return 0, (np.zeros(0, dtype=np.uint64), np.zeros((0, 2), dtype=np.uint8), None)
    for budget, kw, n_pieces in ((env, {}, 8), (explicit, {"hbm_budget": explicit}, 1)):
        et = [_Table(4 ** k, kmer_len=k) for _ in range(N)]
        got = extract.extract_kmers(et[:2], et[2:], call=call, **kw)
        out = max(extract.PIECE_ALIGN * 10, budget // extract.OUTPUT_SHARE)
        assert et[0].reads == _formula(0, 4 ** k, N, budget, out) and got["n_pieces"] == len(et[0].reads) == n_pieces
    assert all(b.freed == 1 for b in device.made)


# ------------------------------------------------------------------ the output writer -------------
def test_atomic_write_renames_after_a_clean_block_only(tmp_path, capsys):
    path = tmp_path / "out.kmq.tsv"
    with output.atomic_write(path, "wt") as fh:
        fh.write("a\tb\n")
        assert not path.exists()
    assert path.read_text() == "a\tb\n" and not (tmp_path / "out.kmq.tsv.tmp").exists()
    assert capsys.readouterr().out == f"saving {path}\n"

    bad = tmp_path / "bad.kmx"
    with pytest.raises(RuntimeError, match="half way"):
        with output.atomic_write(bad, "wb") as fh:
            fh.write(b"\x00")
            raise RuntimeError("half way")
    assert not bad.exists() and capsys.readouterr().out == f"saving {bad}\n"

    meta = tmp_path / "out.json"
    output.write_json(meta, {"b": tmp_path, "a": [1, 2]})
    assert meta.read_text() == json.dumps({"a": [1, 2], "b": str(tmp_path)}, sort_keys=True, indent=1)
    assert capsys.readouterr().out == f"saving {meta}\n" and merger._Encoder is output._Encoder


# ------------------------------------------------------------------ the table-list checks ---------
def test_common_kmer_len_names_the_table_and_the_tool():
    def t(k, name):
        return types.SimpleNamespace(kmer_len=k, index_file=name)
    assert table_list.common_kmer_len([t(9, "a.kin"), t(9, "b.kin")], "query") == 9
    assert table_list.common_kmer_len([], "query") is None
    for tool in ("query", "extract"):
        with pytest.raises(ValueError) as e:
            table_list.common_kmer_len([t(19, "big.kin")], tool)
        assert str(e.value) == f"big.kin: kmer_len 19 is beyond the {tool} path (at most 17: one unsliced table)"
    for k in (0, -1, 8):
        with pytest.raises(ValueError) as e:
            table_list.common_kmer_len([t(9, "a.kin"), t(k, "odd.kin")], "query")
        assert str(e.value) == f"odd.kin: kmer_len {k} is not positive and odd"
    with pytest.raises(ValueError) as e:
        table_list.common_kmer_len([t(9, "a.kin"), t(9, "b.kin"), t(11, "c.kin")], "extract")
    assert str(e.value) == "c.kin: kmer_len 11 differs from the 9 of a.kin"
    sized = types.SimpleNamespace(data_size=4 ** 5, project_name="resident")       # extract's accessor: a table that knows its 4^k
    assert table_list.common_kmer_len([sized], "extract", extract._kmer_len_of) == 5


def test_table_entries_name_the_description_file(tmp_path, capsys):
    assert table_list.description_file("d/s.fa.09.kin.bgz") == table_list.description_file("d/s.fa.09.kin")
    assert str(table_list.description_file("d/s.fa.09.kin")) == "d/s.fa.09.kin.json"
    loaded = []
    entry = table_list.table_entry(3, "d/s.fa.09.kin.bgz", lambda kin: loaded.append(kin) or "header", role="absent")
    assert entry == {"pos": 3, "role": "absent", "index_file": table_list.Path("d/s.fa.09.kin.bgz"),
                     "description_file": table_list.Path("d/s.fa.09.kin.json"), "header": "header"}
    assert loaded == ["d/s.fa.09.kin.bgz"] and capsys.readouterr().out == "verifying d/s.fa.09.kin.bgz\n"
    data = [{"header": types.SimpleNamespace(to_dict=lambda lean: {"lean": lean})}]
    table_list.lean_headers(data)
    assert data == [{"header": {"lean": True}}]
