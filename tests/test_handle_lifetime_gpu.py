"""The handle owns its resources: td_destroy gives back what any entry point allocated on the handle, an
entry point that fails leaves the handle usable, and destroying one handle takes nothing from another."""
import base64
import contextlib
import io
import os

import pytest

from conftest import load_golden, case_payload

pytestmark = pytest.mark.gpu

G = load_golden("splitter.json")
HOT = load_golden("hotpath_cases.json")
ADAPTER = [tuple(x) for x in G["adapters"]["PstI-MspI-Hall"]]

# Device memory that 64 cycles of Engine() / set_splitter / close() may lose beyond what 64 cycles of Engine() / close()
# lose.  A quarter of what the commit before the handle owned its buffers lost, measured once on an MI355X
# (profiles/handle_ownership/lifetime_mi355x.txt: 46 137 344 bytes with a splitter -- the five splitter buffers td_destroy
# did not list -- and 0 without).
LOSS_BOUND = 46137344 // 4
WARM, CYCLES = 8, 64


def splitter_args():
    """384 barcodes and the entries the PstI-MspI-Hall adapter resolves to for them."""
    from tagdigger_amd import tagdigger_fun as tf
    from tagdigger_amd.synth import SynthConfig
    barcodes = SynthConfig(nreads=1, nbar=384, nmarkers=1, seed=7).barcodes
    with contextlib.redirect_stdout(io.StringIO()):
        ends = tf._adapter_ends(ADAPTER, barcodes)
    return barcodes, "TGCAG", ADAPTER[0][0].replace("^", ""), ADAPTER[1][0].replace("^", ""), ends


def lifetime_losses(cycles=CYCLES):
    """(splitter loss, control loss) in bytes of free device memory over `cycles` cycles, each the smaller of two repeats
    (a leak is monotone, what other processes on the card do is not)."""
    import torch
    import tagdigger_amd
    args = splitter_args()

    def cycle(with_splitter):
        eng = tagdigger_amd.Engine(0)
        try:
            if with_splitter:
                eng.set_splitter(*args)
        finally:
            eng.close()

    def loss(with_splitter):
        for _ in range(WARM):
            cycle(with_splitter)
        before = torch.cuda.mem_get_info(0)[0]
        for _ in range(cycles):
            cycle(with_splitter)
        return before - torch.cuda.mem_get_info(0)[0]

    return min(loss(True), loss(True)), min(loss(False), loss(False))


def test_destroy_returns_what_the_splitter_took():
    split, control = lifetime_losses()
    print("free device memory lost over %d cycles: with a splitter %d bytes, without %d bytes" % (CYCLES, split, control))
    assert split - control <= LOSS_BOUND


# ------------------------------------------------------------------------------------------ module states on the handle
# What 64 cycles with a census, a QC, a rescue and a place left open may lose beyond the control: a quarter of the census
# tables alone.  A table is slots x words per slot x 8 bytes, the words per slot by csrc/census.hip's slot_words()
# (2 up to 32 bases, 4 beyond); one table lost per cycle exceeds the bound four times.
CENSUS_SLOTS, CENSUS_TAGLEN = 1 << 20, 20
CENSUS_TABLE_BYTES = CENSUS_SLOTS * (4 if CENSUS_TAGLEN > 32 else 2) * 8
STATE_LOSS_BOUND = CYCLES * CENSUS_TABLE_BYTES // 4


def cutsite_of(case):
    return case["kwargs"].get("cutsite", "TGCAG")


def streaming_cases():
    """The recorded hot-path payloads whose index the census, the QC and the rescue all take and whose file is plain."""
    import rescue_cases as rc
    from oracle import tagdigger_oracle as orc
    out = []
    for c in HOT + load_golden("hotpath_random.json"):
        if "raises" in c or c.get("filename_override") or c["filename"].endswith(".gz") or set(c["kwargs"]) - {"cutsite"}:
            continue
        try:
            barcut, barnum, stored, _ = orc.prepare_lists(c["barcodes"], c["tags"], cutsite_of(c))
            rc.check_tags(stored)
            orc.build_sequence_tree(barcut, barnum)
        except (AssertionError, IndexError, rc.Limit):
            continue
        if rc.part_bases(stored, 1) >= 1:
            out.append(c)
    return out


def smallest_index():
    return min(streaming_cases(), key=lambda c: (len(c["barcodes"]) + len(c["tags"]), sum(map(len, c["tags"]))))


def loss_over(cycle, cycles=CYCLES):
    """Free device memory lost over `cycles` calls of cycle(), the smaller of two repeats (as lifetime_losses)."""
    import torch

    def once():
        for _ in range(WARM):
            cycle()
        before = torch.cuda.mem_get_info(0)[0]
        for _ in range(cycles):
            cycle()
        return before - torch.cuda.mem_get_info(0)[0]

    return min(once(), once())


def test_destroy_returns_what_live_module_states_took():
    import tagdigger_amd
    import place_cases as pc
    c = smallest_index()
    site = min((s for s in pc.site_cases() if pc.site_ref(s[0])["stats"]["loci"]), key=lambda s: len(s[1]))
    G, _, rec_start = pc.parse_fasta(site[1])
    window = pc.site_ref(site[0])["windows"][0]

    def cycle(with_states):
        eng = tagdigger_amd.Engine(0)
        try:
            if with_states:
                eng.census_begin(c["barcodes"], cutsite_of(c), CENSUS_TAGLEN, CENSUS_SLOTS)
                eng.qc_begin(c["barcodes"], cutsite_of(c))
                eng.rescue_begin(c["barcodes"], c["tags"], cutsite_of(c))
                d = eng.dev_alloc(len(G) + 16)
                try:
                    eng.h2d(d, G.encode())
                    place = eng.place_sites(d, len(G), rec_start, pc.remnants_of(site[2]), site[3])
                    eng.place_tags(place, window.encode(), 1, 0)
                    place.ptr = None                                  # left to td_destroy, like the three states
                finally:
                    eng.dev_free(d)
        finally:
            eng.close()

    states, control = loss_over(lambda: cycle(True)), loss_over(lambda: cycle(False))
    print("free device memory lost over %d cycles: with module states %d bytes, without %d bytes; a census table is %d bytes"
          % (CYCLES, states, control, CENSUS_TABLE_BYTES))
    assert states - control <= STATE_LOSS_BOUND


def test_three_streaming_states_on_one_handle(tmp_path):
    """A census, a QC and a rescue on one handle share its readers and its line-prefix scratch: about 40 KiB of recorded
    reads (three 16 KiB tiles) as a file and as a device buffer to each of them in turn, the QC ended in between; every
    fetch equals what a fresh handle gives that runs the module alone over the same inputs."""
    import tagdigger_amd
    c = next(c for c in streaming_cases() if c["name"] == "random043")
    payload = case_payload(c)
    assert payload.endswith(b"\n")
    data = payload * (40 * 1024 // len(payload) + 1)
    assert 2 * 16384 < len(data) <= 3 * 16384
    path = os.path.join(str(tmp_path), "three.fq")
    with open(path, "wb") as fh:
        fh.write(data)
    args = (c["barcodes"], cutsite_of(c))

    def census(eng):
        seqs, counts = eng.census_fetch()
        return seqs, counts, eng.census_stats()

    def qc(eng):
        return [t.tolist() for t in eng.qc_fetch()], eng.qc_stats()

    def rescue(eng):
        matrix, pos = eng.rescue_fetch()
        return matrix.tolist(), pos.tolist(), eng.rescue_stats()

    def run(eng, mods):
        """The sequence of the docstring for the modules of `mods`; the fetches in the order made."""
        got = []
        if "census" in mods:
            eng.census_begin(*args, 20, 4096)
        if "qc" in mods:
            eng.qc_begin(*args)
        if "rescue" in mods:
            eng.rescue_begin(c["barcodes"], c["tags"], cutsite_of(c), 2)
        d = eng.dev_alloc(len(data))
        try:
            eng.h2d(d, data)
            for m in mods:
                getattr(eng, m + "_file")(path)
            for m in mods + mods[::-1]:
                getattr(eng, m + "_device")(d, len(data))
            eng.sync()
            for m in mods:
                got.append((m, fetchers[m](eng)))
            if "qc" in mods:
                eng.qc_end()
            for m in mods:
                if m != "qc":
                    getattr(eng, m + "_device")(d, len(data))
            eng.sync()
            for m in mods:
                if m != "qc":
                    got.append((m, fetchers[m](eng)))
        finally:
            eng.dev_free(d)
        return got

    fetchers = dict(census=census, qc=qc, rescue=rescue)
    together = tagdigger_amd.Engine(0)
    try:
        got = run(together, ["census", "qc", "rescue"])
    finally:
        together.close()
    assert [m for m, _ in got] == ["census", "qc", "rescue", "census", "rescue"]
    import census_cases
    once = census_cases.ref_census(data, *args, 20)[1]                                # one file pass and two device passes
    assert got[0][1][2]["reads"] == 3 * once["reads"] and got[0][1][2]["counted"] == 3 * once["counted"] > 0
    assert got[2][1][2]["rescued1"] > 0 and got[1][1][1]["reads"] == got[0][1][2]["reads"]
    for m in ("census", "qc", "rescue"):
        alone = tagdigger_amd.Engine(0)
        try:
            assert run(alone, [m]) == [g for g in got if g[0] == m], m
        finally:
            alone.close()


FILE_CALLS = {
    # module -> (begin, fetch) on an engine; the C-ABI's td_<mod>_file and td_<mod>_stats are called by name
    "census": (lambda eng, c: eng.census_begin(c["barcodes"], cutsite_of(c), 20, 1024),
               lambda eng: (eng.census_fetch(), eng.census_stats())),
    "qc": (lambda eng, c: eng.qc_begin(c["barcodes"], cutsite_of(c)),
           lambda eng: (eng.qc_fetch(), eng.qc_stats())),
    "rescue": (lambda eng, c: eng.rescue_begin(c["barcodes"], c["tags"], cutsite_of(c)),
               lambda eng: ([a.tolist() for a in eng.rescue_fetch()], eng.rescue_stats())),
}


def golden_result(mod, c):
    """What the module's restated rule gives for the recorded payload."""
    import census_cases
    import qc_cases
    import rescue_cases as rc
    data = case_payload(c)
    if mod == "census":
        census, st = census_cases.ref_census(data, c["barcodes"], cutsite_of(c), 20)
        return census_cases.ordered(census), st
    if mod == "qc":
        return qc_cases.ref_qc(data, c["barcodes"], cutsite_of(c))
    rescued, st, positions, _ = rc.ref_rescue(data, c["barcodes"], c["tags"], cutsite_of(c))
    return rescued, st, positions


def same_as_golden(mod, got, want):
    import qc_cases
    import rescue_cases as rc
    if mod == "census":
        (lists, st), (wlists, wst) = got, want
        assert tuple(lists) == tuple(wlists) and all(st[k] == wst[k] for k in ("reads", "barcut", "short", "ambiguous", "counted", "distinct"))
    elif mod == "qc":
        tables, st = got
        qc_cases.same(dict(zip(qc_cases.TABLES, tables), stats=st), want)
    else:
        (matrix, positions), st = got
        assert matrix == want[0] and positions == want[2] and {k: st[k] for k in rc.CLASSES} == want[1]


@pytest.mark.parametrize("mod", sorted(FILE_CALLS))
def test_a_path_that_does_not_exist(mod, tmp_path):
    """td_<mod>_file on a missing path is TD_E_IO.  On a fresh state nothing is latched and a good file still gives the
    golden result; after a good file the tables would hold a part of two files, so every call answers TD_E_IO with the same
    text until the next begin."""
    import ctypes as C
    import tagdigger_amd
    c = next(c for c in streaming_cases() if c["name"] == "random043")
    good = os.path.join(str(tmp_path), "good.fq")
    with open(good, "wb") as fh:
        fh.write(case_payload(c))
    missing = os.path.join(str(tmp_path), "nowhere", "reads.fq").encode()
    begin, fetch = FILE_CALLS[mod]
    eng = tagdigger_amd.Engine(0)
    L = eng._L
    file_, stats, st = getattr(L, "td_%s_file" % mod), getattr(L, "td_%s_stats" % mod), (C.c_uint64 * 8)()
    try:
        begin(eng, c)
        assert file_(eng._h, missing, 2 ** 62) == -11                                 # TD_E_IO, nothing added before
        assert stats(eng._h, st) == 0
        assert file_(eng._h, good.encode(), 2 ** 62) == 0
        same_as_golden(mod, fetch(eng), golden_result(mod, c))
        assert file_(eng._h, missing, 2 ** 62) == -11                                 # ... and after a good file
        msg = L.td_last_error()
        assert msg
        for _ in range(2):
            assert stats(eng._h, st) == -11 and L.td_last_error() == msg
        assert file_(eng._h, good.encode(), 2 ** 62) == -11 and L.td_last_error() == msg
        with pytest.raises(tagdigger_amd.TagdigError) as ei:
            fetch(eng)
        assert ei.value.code == -11 and ei.value.detail == msg.decode()
        begin(eng, c)
        assert file_(eng._h, good.encode(), 2 ** 62) == 0 and stats(eng._h, st) == 0
        same_as_golden(mod, fetch(eng), golden_result(mod, c))
    finally:
        eng.close()


def good_split_cases():
    return [c for c in G["split"] if "raises" not in c and not c["gz"]]


def split_through(eng, c, directory, outs=None):
    """The case's input split by `eng` into files under `directory`; the files' bytes in base64 (None: not there)."""
    from tagdigger_amd import tagdigger_fun as tf
    ad = [tuple(x) for x in G["adapters"][c["adapter"]]]
    with contextlib.redirect_stdout(io.StringIO()):
        ends = tf._adapter_ends(ad, c["barcodes"])
    eng.set_splitter(c["barcodes"], c["cutsite"], ad[0][0].replace("^", ""), ad[1][0].replace("^", ""), ends)
    src = os.path.join(str(directory), "in.fq")
    with open(src, "wb") as fh:
        fh.write(base64.b64decode(c["fastq_b64"]))
    outs = outs or [os.path.join(str(directory), "out%d.fq" % i) for i in range(len(c["barcodes"]))]
    kw = {} if c["maxreads"] is None else {"maxreads": c["maxreads"]}
    eng.split_file(src, outs, **kw)
    return [base64.b64encode(open(o, "rb").read()).decode() for o in outs]


def test_refused_split_file_leaves_the_handle_usable(tmp_path):
    """The smallest good case (an empty input) and the smallest with reads: an output path in a directory that does not
    exist is TD_E_IO, and the same engine then splits the same case into the golden bytes."""
    import tagdigger_amd
    from tagdigger_amd._binding import TagdigError
    by_size = sorted(good_split_cases(), key=lambda c: len(c["fastq_b64"]))
    cases = [by_size[0], next(c for c in by_size if c["fastq_b64"])]
    eng = tagdigger_amd.Engine(0)
    try:
        for k, c in enumerate(cases):
            d = tmp_path / str(k)
            d.mkdir()
            outs = [str(d / ("out%d.fq" % i)) for i in range(len(c["barcodes"]))]
            bad = list(outs)
            bad[-1] = str(d / "nowhere" / "out.fq")
            with pytest.raises(TagdigError) as ei:
                split_through(eng, c, d, bad)
            assert ei.value.code == -11                       # TD_E_IO
            assert split_through(eng, c, d, outs) == c["outputs_b64"]
    finally:
        eng.close()


def test_two_handles_interleaved(tmp_path):
    import tagdigger_amd
    hot = HOT[0]
    gz = min((c for c in HOT if c["filename"].endswith(".gz") and "raises" not in c and not c["kwargs"]), key=lambda c: len(c["fastq_b64"]))
    a, b = tagdigger_amd.Engine(0), tagdigger_amd.Engine(0)
    try:
        for eng in (a, b):
            eng.set_index(hot["barcodes"], hot["tags"], hot["kwargs"].get("cutsite", "TGCAG"))
            eng.count_bytes(case_payload(hot))
        assert a.counts() == hot["counts"] and b.counts() == hot["counts"]
        a.close()
        path = os.path.join(str(tmp_path), gz["filename"])
        with open(path, "wb") as fh:
            fh.write(case_payload(gz))
        b.set_index(gz["barcodes"], gz["tags"], "TGCAG")
        b.count_file(path)
        assert b.counts() == gz["counts"]
        split = good_split_cases()[0]
        assert split_through(b, split, tmp_path) == split["outputs_b64"]
    finally:
        a.close()
        b.close()
