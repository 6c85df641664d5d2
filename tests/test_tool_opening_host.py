"""CPU: the order of the refusals with which query(), filter() and mask() open, where a run is wrong in several ways at once:
an existing output before a missing input, a missing input before anything about the tables, a table's file before the count
window.  Nothing here reaches a device: every run is refused first."""
import pytest

from pykmer_amd import filter as kfilter, mask, query

TOOLS = {"query": (query.query, ".kmq.tsv", {}), "binned query": (query.query, ".kmb.json", {"bin_windows": 4}),
         "filter": (kfilter.filter, ".kmf", {}), "mask": (mask.mask, ".kmm.json", {})}


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_outputs_then_inputs_then_tables_then_the_count_window(tool, tmp_path):
    run, ext, kw = TOOLS[tool]
    proj, q, missing = str(tmp_path / "p"), tmp_path / "q.fa", tmp_path / "none.fa"
    q.write_bytes(b">r\nACGTACGTACGT\n")
    no_kin, bad_kin = tmp_path / "none.kin", tmp_path / "t.txt"
    mine = tmp_path / ("p" + ext)
    mine.write_bytes(b"mine")
    with pytest.raises(ValueError, match="already exists"):
        run(proj, str(missing), [no_kin], min_count=9, max_count=3, **kw)
    mine.unlink()
    with pytest.raises(ValueError, match="query file does not exist"):
        run(proj, str(missing), [no_kin], min_count=9, max_count=3, **kw)
    with pytest.raises(ValueError, match="table file does not exist"):
        run(proj, str(q), [no_kin], min_count=9, max_count=3, **kw)
    with pytest.raises(ValueError, match="all tables must be"):
        run(proj, str(q), [bad_kin, no_kin], min_count=9, max_count=3, **kw)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["q.fa"]


def test_what_each_tool_checks_before_it_looks_at_a_file(tmp_path):
    proj, missing = str(tmp_path / "p"), str(tmp_path / "none.fa")
    many = [tmp_path / f"none{i}.kin" for i in range(query.MAX_PAIR_TABLES + 1)]
    for ext in (".kmq", ".kmf", ".kmm"):
        (tmp_path / ("p" + ext)).write_bytes(b"mine")
    # query: its options before the outputs; the number of tables behind the outputs and the query file, before any table
    with pytest.raises(ValueError, match="--coords"):
        query.query(proj, missing, many, coords=True)
    with pytest.raises(ValueError, match="already exists"):
        query.query(proj, missing, many, pairs=True)
    with pytest.raises(ValueError, match="already exists"):
        query.query(proj, missing, [])
    (tmp_path / "p.kmq").unlink()
    with pytest.raises(ValueError, match="query file does not exist"):
        query.query(proj, missing, many, pairs=True)
    with pytest.raises(ValueError, match="query file does not exist"):
        query.query(proj, missing, [])
    q = tmp_path / "q.fa"
    q.write_bytes(b">r\nACGT\n")
    with pytest.raises(ValueError, match="--pairs takes at most"):
        query.query(proj, str(q), many, pairs=True)
    with pytest.raises(ValueError, match="a query needs at least one table"):
        query.query(proj, str(q), [])
    # filter: the rule and the number of tables before the outputs
    with pytest.raises(ValueError, match="a filter needs at least one table"):
        kfilter.filter(proj, missing, [])
    with pytest.raises(ValueError, match="--min-tables"):
        kfilter.filter(proj, missing, many[:2], min_tables=3)
    with pytest.raises(ValueError, match="already exists"):
        kfilter.filter(proj, missing, many[:2])
    # mask: the input's format and the number of tables before the outputs
    with pytest.raises(ValueError, match="takes FASTA input"):
        mask.mask(proj, str(tmp_path / "none.fq"), [])
    with pytest.raises(ValueError, match="a mask needs at least one table"):
        mask.mask(proj, missing, [])
    with pytest.raises(ValueError, match="already exists"):
        mask.mask(proj, missing, many[:2])
