#!/usr/bin/env python3
"""Generate tests/golden/splitter_edges.json from the REAL reference (build container only; data only, never
reference code): for every adapter/barcode set of tests/splitter_edge_cases.py, its edge reads (as the specs they are
built from) and the reference's own answers -- the barcode index from sequence_index_lookup over barcode + cut site,
and findAdapterSeq's value -- on the text the reference's record loop would hand them (line.strip().upper()).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_splitter_edges_golden.py [/root/reference]
"""
import contextlib
import io
import itertools
import json
import os
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))                      # tests/: the case builders
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository: the builders import the oracle (not used here)
import tagdigger_fun as ref  # noqa: E402
import splitter_edge_cases as ec  # noqa: E402


def main():
    sets = {}
    nreads = 0
    for name, reads in ec.edge_reads().items():
        st = ec.SETS[name]
        adapter = [tuple(x) for x in st.adapter]
        barcut = ref.combine_barcode_and_cutsite(st.barcodes, st.cutsite)
        tree = ref.build_sequence_tree(barcut, len(barcut))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            trees = ref.build_adapter_tree(adapter, st.barcodes)
        site0, site1 = adapter[0][0].replace("^", ""), adapter[1][0].replace("^", "")
        bars, values = [], []
        for _, spec in reads:
            seq = ec.expand(spec).strip().upper()
            bar = ref.sequence_index_lookup(seq, tree)
            bars.append(bar)
            values.append(ref.findAdapterSeq(seq, trees[bar], site0, site1, len(st.barcodes[bar]) + len(st.cutsite)) if bar > -1 else None)
        sets[name] = {"adapter": [list(x) for x in adapter], "barcodes": st.barcodes, "cutsite": st.cutsite, "stdout": buf.getvalue(),
                      "groups": [[g, len(list(run))] for g, run in itertools.groupby(g for g, _ in reads)],
                      "specs": [s for _, s in reads], "bar": bars, "values": values}
        nreads += len(reads)
    path = os.path.join(HERE, "splitter_edges.json")
    with open(path, "w") as fh:
        json.dump({"sets": sets}, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote splitter_edges.json:", len(sets), "sets,", nreads, "reads,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
