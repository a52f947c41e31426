"""The splitter's edge cases on the CPU (tests/splitter_edge_cases.py): the builders' self-checks, the oracle's
restatement against the real reference's answers on every edge read (tests/golden/splitter_edges.json, written by
tests/golden/make_splitter_edges_golden.py), and the product's host-side entry lists against the sets the cases
assume.  tests/test_splitter_edges_gpu.py then holds both kernels against the oracle on the same buffers."""
import contextlib
import io

import pytest

import splitter_edge_cases as ec
from conftest import load_golden

G = load_golden("splitter_edges.json")["sets"]


def test_builders_have_the_properties_they_are_named_for():
    assert ec.self_checks()


def test_golden_holds_the_reads_the_builders_make():
    """The fixture and the builders cannot drift apart: same sets, same settings, same reads in the same order."""
    reads = ec.edge_reads()
    assert list(G) == list(reads) and sorted(G) == sorted(ec.SETS)
    for name, g in G.items():
        st = ec.SETS[name]
        assert [tuple(x) for x in g["adapter"]] == [tuple(x) for x in st.adapter]
        assert g["barcodes"] == st.barcodes and g["cutsite"] == st.cutsite
        assert g["specs"] == [s for _, s in reads[name]]
        assert [x for x, n in g["groups"] for _ in range(n)] == [x for x, _ in reads[name]]
        assert len(g["bar"]) == len(g["values"]) == len(g["specs"])


@pytest.mark.parametrize("name", list(ec.SETS))
def test_oracle_equals_the_reference_on_every_edge_read(name):
    g = G[name]
    st = ec.SETS[name]
    log = []
    ec.po.build_adapter_tree(st.adapter, st.barcodes, log)
    assert "".join(x + "\n" for x in log) == g["stdout"]
    got = ec.oracle_decisions(st, [ec.expand(s) for s in g["specs"]])
    want = list(zip(g["bar"], g["values"]))
    assert got == want, [(s, a, b) for s, a, b in zip(g["specs"], got, want) if a != b][:5]


@pytest.mark.parametrize("name", list(ec.SETS))
def test_adapter_ends_are_the_entry_sets_the_cases_assume(name):
    """tf._adapter_ends -- what the product hands to td_set_splitter -- holds the entries of the oracle's trie, so the
    group sizes and entry lengths the builders checked are those the library sees."""
    from tagdigger_amd import tagdigger_fun as tf
    st = ec.SETS[name]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ends = tf._adapter_ends(st.adapter, st.barcodes)
    assert buf.getvalue() == G[name]["stdout"]
    assert [sorted(per) for per in ends] == ec.entries_from_oracle(st)
    assert ec.compact_form(st, ends) == st.compact


@pytest.mark.parametrize("name", list(ec.cases()))
def test_case_buffers_and_their_expected_decisions(name):
    """Every buffer: as many expected decisions as it has sequence lines, for a buffer that starts on a header line and
    for the same bytes cut to begin at their first sequence line; the read cases' decisions are the golden's."""
    c = ec.cases()[name]
    data = ec.ascii_twin(c.data) if c.error is None else None
    if data is None:
        return
    want = ec.expected(c.set, data)
    assert len(want) == ec.seq_line_count(c.data, 0) == ec.seq_line_count(c.data, 4)
    lines = ec.lines_of(c.data)
    if len(lines) > 1 or c.data[-1:] in (b"\n", b"\r"):
        cut = len(lines[0]) + (2 if c.data[len(lines[0]):len(lines[0]) + 2] == b"\r\n" else 1)
        assert ec.seq_line_count(c.data[cut:], 1) == len(want)
    if c.labels is not None:
        assert len(c.labels) == len(want)
    if name in G or name in ("hall-A", "hall-B", "hall-B-crlf"):
        g = G[c.set]
        groups = [x for x, n in g["groups"] for _ in range(n)]
        keep = [k for k, x in enumerate(groups) if name in G or x.split("-")[0] == name.split("-")[1]]
        assert want[1:-1] == [(g["bar"][k], 999 if g["bar"][k] < 0 else g["values"][k]) for k in keep]     # (between lead and trail)
