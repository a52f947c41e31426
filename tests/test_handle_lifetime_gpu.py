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
