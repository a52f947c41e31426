"""The BGZF batch feeder (BgzfFeeder in csrc/tagdig.hip) at a batch size small enough that a small file takes several batches: 200
members of 1 KiB of FASTQ and the end-of-file member, option zb_members = 64, so every call walks four batches and
uses both pinned staging pieces and both batch slots twice.  td_bgzf_inflate_range (multi-GPU: a rank's members) and
td_count_file's BGZF route share the feeder; the ranges must come back byte for byte, the counts must be the C oracle's.
"""
import os
import random
import re

import pytest
import torch

from helpers import bgzf_bytes, dirty_fastq, small_index
from oracle import c_oracle

pytestmark = pytest.mark.gpu

MEMBER = 1024
BATCH = 64


@pytest.fixture(scope="module")
def lib():
    """(barcodes, tags, text, BGZF bytes): the text is cut at a line end so that it fills 200 members."""
    rnd = random.Random(20)
    barcodes, tags, cutsites = small_index(rnd, "TGCAG", nbar=6, ntag=30)
    data = dirty_fastq(rnd, barcodes, tags, cutsites, nrec=2500)
    assert len(data) > 200 * MEMBER
    data = data[:data.rindex(b"\n", 0, 200 * MEMBER) + 1]
    blob = bgzf_bytes(data, block=MEMBER)
    return barcodes, tags, data, blob


@pytest.fixture()
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    e.set_option("zb_members", BATCH)
    yield e
    e.set_option("zb_members", 1 << 30)
    e.close()


def write(tmp_path, name, blob):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(blob)
    return path


def index(path):
    from tagdigger_amd import multi
    moff, misz = multi.bgzf_index(path)
    return [int(x) for x in moff], [int(x) for x in misz]


def inflate(eng, path, begin, end, capacity):
    dst = torch.zeros(capacity + 64, dtype=torch.uint8, device="cuda:0")
    n = eng.bgzf_inflate_range(path, begin, end, dst.data_ptr(), capacity)
    return bytes(dst[:n].cpu().numpy())


def test_whole_file_range(eng, lib, tmp_path):
    _, _, data, blob = lib
    path = write(tmp_path, "whole.fq.gz", blob)
    moff, misz = index(path)
    assert 3 * BATCH < len(moff) <= 4 * BATCH and sum(misz) == len(data)       # four batches
    assert inflate(eng, path, 0, len(blob), len(data)) == data


def test_sub_ranges_share_no_state(eng, lib, tmp_path):
    """[off_k, off_m) across a batch boundary and short of the last member, then another range on the same handle."""
    _, _, data, blob = lib
    path = write(tmp_path, "sub.fq.gz", blob)
    moff, misz = index(path)
    text_at = [0]
    for s in misz:
        text_at.append(text_at[-1] + s)
    for k, m in ((37, 37 + BATCH + 30), (5, 5 + 2 * BATCH + 1), (150, 151)):
        assert m < len(moff) - 1                                               # (ends before the last member)
        want = data[text_at[k]:text_at[m]]
        assert inflate(eng, path, moff[k], moff[m], len(want)) == want


def test_trailing_zero_padding(eng, lib, tmp_path):
    """64 zero bytes behind the end-of-file member: td_count_file reads the file as gzip.open does (the padding is no
    data); a range that reaches into the padding is refused, one that ends in front of it is served."""
    from tagdigger_amd._binding import TagdigError
    barcodes, tags, data, blob = lib
    path = write(tmp_path, "padded.fq.gz", blob + bytes(64))
    ost = {}
    want = c_oracle.COracle(barcodes, tags, "TGCAG").count_bytes(data, stats=ost)
    eng.set_index(barcodes, tags, "TGCAG")
    eng.count_file(path)
    st = eng.stats()
    assert (eng.counts_numpy() == want).all()
    assert (st["reads"], st["barcut"], st["tag"]) == (ost["reads"], ost["barcut"], ost["tag"])
    with pytest.raises(TagdigError, match="damaged BGZF member header"):
        inflate(eng, path, 0, len(blob) + 64, len(data))
    assert inflate(eng, path, 0, len(blob), len(data)) == data


def test_maxreads_inside_the_second_batch(eng, lib, tmp_path):
    """The bound falls into the second of four batches: the matrix and the counters are the oracle's for that bound."""
    barcodes, tags, data, blob = lib
    path = write(tmp_path, "bound.fq.gz", blob)
    # line k of the text starts at starts[k] (terminators by the reference's rule: \r\n is one)
    starts = [0] + [m.end() for m in re.finditer(rb"\r\n|\r|\n", data)]
    maxreads = next(r for r in range(1, len(starts) // 4) if starts[4 * (r - 1) + 1] >= BATCH * MEMBER * 3 // 2)
    assert BATCH * MEMBER < starts[4 * (maxreads - 1) + 1] < 2 * BATCH * MEMBER
    ost = {}
    want = c_oracle.COracle(barcodes, tags, "TGCAG").count_bytes(data, maxreads=maxreads, stats=ost)
    assert ost["reads"] == maxreads and want.sum() > 0
    eng.set_index(barcodes, tags, "TGCAG")
    eng.count_file(path, maxreads=maxreads)
    st = eng.stats()
    assert (eng.counts_numpy() == want).all()
    assert (st["reads"], st["barcut"], st["tag"]) == (ost["reads"], ost["barcut"], ost["tag"])
