"""The catalogue of tests/deflate_cases.py -- DEFLATE streams that no zlib encoder writes, and streams zlib refuses -- against
zlib itself, against a reader of this file's own (the structure every case claims is read back out of its bits), and through
the three host decoders: fast_inflate.hpp and both forms of par_inflate.hpp (td_gunzip_file) and the host build of the lane
decoder gpu_inflate.hpp (td_inflate_raw_host).  tests/test_deflate_edges_gpu.py takes the same catalogue to the device."""
import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_cases as dc

CASES = dc.catalogue()
VALID, REFUSED = dc.valid_names(), dc.refused_names()
SMALL = [n for n, c in CASES.items() if len(c.trailer_text) <= 65536 and len(c.raw) <= 65536 - 26]      # (the lane decoder's: one BGZF member)


# ---------------------------------------------------------------------------------------------- a DEFLATE reader of its own
class Reader:
    """RFC 1951 read back: every block's header fields, its code-length sequence as it was spelled, its lengths, and every
    token with its bit offset and size.  ValueError for what the RFC does not allow."""

    _luts = {}

    def __init__(self, raw):
        self.raw = raw + bytes(16)
        self.pos = 0
        self.blocks = []
        self.text = bytearray()

    def peek(self, n):
        return (int.from_bytes(self.raw[self.pos >> 3:(self.pos >> 3) + 8], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.pos += n
        return v

    @classmethod
    def lut(cls, lengths):
        """low bits of the stream -> (symbol, code length), for a set of lengths that is not over-subscribed"""
        key = tuple(lengths)
        if key not in cls._luts:
            if sum(1 << (15 - l) for l in lengths if l) > 32768:
                raise ValueError("over-subscribed")
            mx = max(lengths) if any(lengths) else 0
            table = [None] * (1 << mx)
            code = 0
            for bits in range(1, mx + 1):
                for sym, l in enumerate(lengths):
                    if l == bits:
                        rev = int(format(code, "0%db" % bits)[::-1], 2)
                        for k in range(rev, 1 << mx, 1 << bits):
                            table[k] = (sym, bits)
                        code += 1
                code <<= 1
            cls._luts[key] = (table, mx)
        return cls._luts[key]

    @staticmethod
    def allowed(lengths, code_lengths=False):
        """zlib's rule (inftrees.c): no set may be over-subscribed, and an incomplete one is allowed only as a single code of
        one bit (or no code at all) for literal/length or distance symbols"""
        k = sum(1 << (15 - l) for l in lengths if l)
        if k > 32768 or (k < 32768 and (code_lengths or max(lengths) > 1)):
            raise ValueError("over-subscribed or incomplete set of lengths")

    def symbol(self, lut):
        table, mx = lut
        e = table[self.peek(mx)] if mx else None
        if e is None:
            raise ValueError("no such code")
        self.pos += e[1]
        return e[0]

    def block(self, header_only=False):
        b = dict(bit=self.pos, final=self.take(1), type=self.take(2), tokens=[], out=len(self.text))
        self.blocks.append(b)
        if b["type"] == 3:
            raise ValueError("block type 3")
        if b["type"] == 0:
            self.pos += -self.pos % 8
            b["len"], nlen = self.take(16), self.take(16)
            if b["len"] ^ nlen != 0xFFFF:
                raise ValueError("LEN / NLEN")
            b["data"] = self.pos >> 3
            self.text += self.raw[b["data"]:b["data"] + b["len"]]
            self.pos += 8 * b["len"]
            return b
        if b["type"] == 1:
            litlen, dist = dc.FIXED_LITLEN, dc.FIXED_DIST
        else:
            b["hlit"], b["hdist"], b["hclen"] = self.take(5) + 257, self.take(5) + 1, self.take(4) + 4
            if b["hlit"] > 286 or b["hdist"] > 30:
                raise ValueError("too many symbols")
            cl = [0] * 19
            for s in dc.CL_ORDER[:b["hclen"]]:
                cl[s] = self.take(3)
            b["cl_lengths"] = cl
            self.allowed(cl, True)
            lut = self.lut(cl)
            seq, spelled = [], []
            while len(seq) < b["hlit"] + b["hdist"]:
                s = self.symbol(lut)
                at = len(seq)
                if s < 16:
                    seq.append(s)
                    spelled.append((at, s, 1))
                    continue
                if s == 16:
                    if not seq:
                        raise ValueError("repeat with no previous length")
                    n, v = 3 + self.take(2), seq[-1]
                elif s == 17:
                    n, v = 3 + self.take(3), 0
                else:
                    n, v = 11 + self.take(7), 0
                seq += [v] * n
                spelled.append((at, s, n))
            if len(seq) > b["hlit"] + b["hdist"]:
                raise ValueError("a repeat runs past the lengths")
            b["spelled"] = spelled
            litlen, dist = seq[:b["hlit"]], seq[b["hlit"]:]
            if not litlen[256]:
                raise ValueError("no end code")
            self.allowed(litlen)
            self.allowed(dist)
        b["litlen"], b["dist"] = list(litlen), list(dist)
        if header_only:
            return b
        ll, dl = self.lut(litlen), self.lut(dist)
        text, tokens = self.text, b["tokens"]
        while True:
            at = self.pos
            s = self.symbol(ll)
            if s < 256:
                text.append(s)
                tokens.append((at, self.pos - at, s, 0, 0))
                continue
            if s == 256:
                break
            if s > 285:
                raise ValueError("length symbol")
            length = dc.LENGTH_BASE[s - 257] + self.take(dc.LENGTH_EXTRA[s - 257])
            d = self.symbol(dl)
            if d > 29:
                raise ValueError("distance symbol")
            distance = dc.DIST_BASE[d] + self.take(dc.DIST_EXTRA[d])
            if distance > len(text):
                raise ValueError("too far back")
            tokens.append((at, self.pos - at, s, length, distance))
            src = len(text) - distance
            if distance >= length:
                text += text[src:src + length]
            else:
                text += (bytes(text[src:]) * (length // distance + 1))[:length]
        return b

    def run(self):
        while not self.block()["final"]:
            pass
        return self


_PARSED = {}


def parsed(name):
    if name not in _PARSED:
        _PARSED[name] = Reader(CASES[name].raw).run()
    return _PARSED[name]


def complete(lengths):
    return sum(1 << (15 - l) for l in lengths if l) == 32768


def copies(block):
    return [(t[3], t[4]) for t in block["tokens"] if t[3]]


def lanes_of(block):
    """the lane of a step of the wave decoder (64 bit positions from where the step before ended) each token starts at"""
    out, step = [], block["tokens"][0][0]
    for t in block["tokens"]:
        if t[0] - step >= 64:
            step = t[0]
        out.append(t[0] - step)
    return out


# ---------------------------------------------------------------------------------------------- the catalogue itself
@pytest.mark.parametrize("name", list(CASES))
def test_catalogue_against_zlib(name):
    c = CASES[name]
    if c.want is None:
        with pytest.raises(zlib.error):
            zlib.decompress(c.raw, -15)
        with pytest.raises(ValueError):
            Reader(c.raw).run()
    else:
        d = zlib.decompressobj(-15)
        assert d.decompress(c.raw) == c.want and d.eof and d.unused_data == b""
        r = parsed(name)
        assert bytes(r.text) == c.want
        assert (r.pos + 7) // 8 == len(c.raw)
        assert sum(len(b["tokens"]) + b.get("len", 0) for b in r.blocks) == c.ntokens
        assert [(b["bit"], b["type"]) for b in r.blocks] == c.blocks


def test_the_device_rule_holds_for_the_catalogue():
    """What gz_gpu.hpp may leave to the host: files under 64 bytes, an incomplete literal/length code, a chunk with more tokens
    than 4 * span + 4096, small members, no room.  Every case marked device=True is out of the reach of the first three."""
    for name in VALID:
        c = CASES[name]
        if not c.device:
            assert c.why
            continue
        assert len(c.member()) >= 64
        assert c.ntokens + 192 <= 4 * len(c.raw) + 4096
        for b in parsed(name).blocks:
            if b["type"] == 2:
                assert complete(b["litlen"]), name
    assert [n for n in VALID if not CASES[n].device] == ["only-end-code"]
    names = set(CASES)
    assert {"long-codes-max-tokens", "258-as-284-31", "dist-32768-exact", "one-distance-code", "no-distance-code", "repeat-across-lit-dist",
            "empty-blocks-alignments", "stored-65535-then-copies", "overlapping-copies", "dependent-copies", "empty-text-64",
            "only-end-code", "many-chunks", "decoy-in-stored"} <= set(VALID)
    assert {"dist-too-far", "copy-from-nothing", "toofar-zero-trailer", "repeat-with-no-previous", "fixed-symbol-286", "fixed-distance-30",
            "oversubscribed-litlen", "incomplete-litlen", "distance-used-but-none-defined", "block-type-3", "stored-len-nlen", "hlit-287",
            "no-end-of-block-code"} <= set(REFUSED) <= names


@pytest.mark.parametrize("name", ["long-codes-max-tokens", "long-codes-small"])
def test_long_codes(name):
    r = parsed(name)
    ladder = list(range(1, 15)) + [15, 15]
    for b, lsym, size in zip(r.blocks, (285, 284) if name == "long-codes-max-tokens" else (284,), (43, 48) if name == "long-codes-max-tokens" else (48,)):
        assert b["type"] == 2
        assert sorted(l for l in b["litlen"] if l) == ladder and b["litlen"][256] == 15 and b["litlen"][lsym] == 15
        assert sorted(l for l in b["dist"] if l) == ladder and b["dist"][29] == 15
        big = [t for t in b["tokens"] if t[3]]
        assert all(t[3] == 258 and t[2] == lsym and 24577 <= t[4] <= 32768 and t[1] == size for t in big)
        assert {32768, 24577} <= {t[4] for t in big}
        between = [t[1] for t in b["tokens"] if not t[3] and t[0] > big[0][0]]
        assert 14 in between and max(between) == 14
    first = r.blocks[0]["tokens"]
    prefix = first[:[i for i, t in enumerate(first) if t[3]][0]]
    assert sum(t[1] <= 10 for t in prefix) >= 32768                                          # 32 KiB of short-code literals first
    if name == "long-codes-small":
        return
    for b, size in zip(r.blocks, (43, 48)):
        big = [t for t in b["tokens"] if t[3]]
        assert len(big) >= 300
        assert {t[0] % 64 for t in big} == set(range(64))                                      # every bit offset of two words
        assert {lane for lane, t in zip(lanes_of(b), b["tokens"]) if t[3]} == set(range(64))   # every lane of a step
    # the five-word path: a token of the full 48 bits that starts in bits 1985 ... 2047 of a 2048-bit block of the FILE (the
    # decoder's registers hold the file from a multiple of 4 KiB on; the member's header is 10 bytes)
    assert [t for t in r.blocks[1]["tokens"] if t[1] == 48 and 1985 <= (80 + t[0]) % 2048 <= 2047]


def test_258_as_284_31():
    (b,) = parsed("258-as-284-31").blocks
    assert b["type"] == 1
    assert len([t for t in b["tokens"] if t[2] == 284 and t[3] == 258]) >= 3 and not [t for t in b["tokens"] if t[2] == 285]


def test_dist_32768_exact():
    r = parsed("dist-32768-exact")
    assert r.blocks[1]["out"] == 32768 and r.blocks[1]["tokens"][0][3:] == (258, 32768)         # its source begins at byte 0
    assert not copies(r.blocks[0])
    # (and the refused twin: one byte of text less in front of the same copy)
    with pytest.raises(zlib.error, match="too far back"):
        zlib.decompress(CASES["dist-too-far"].raw, -15)
    assert zlib_produced(CASES["dist-too-far"].raw) == 32767


def test_one_and_no_distance_code():
    (b,) = parsed("one-distance-code").blocks
    assert b["type"] == 2 and b["hdist"] == 1 and b["dist"] == [1] and {d for _, d in copies(b)} == {1}
    (b,) = parsed("no-distance-code").blocks
    assert b["type"] == 2 and b["hdist"] == 1 and b["dist"] == [0] and not copies(b)


def test_repeat_across_the_boundary():
    b1, b2, b3 = parsed("repeat-across-lit-dist").blocks
    assert (b1["hlit"], b2["hlit"], b3["hlit"]) == (258, 286, 257) and (b1["hclen"], b2["hclen"], b3["hclen"]) == (19, 19, 5)
    crossing = [(at, s, n) for at, s, n in b1["spelled"] if s == 16 and at < b1["hlit"] < at + n]
    assert crossing and crossing[0][0] == 257 and crossing[0][2] == 6                            # 257 and five distance lengths
    assert [x for x in b2["spelled"] if x[1:] == (18, 138)] and [t for t in b2["tokens"] if t[2] == 285]
    assert all(complete(b[k]) for b in (b1, b2, b3) for k in ("cl_lengths", "litlen")) and complete(b1["dist"])
    assert sorted(l for l in b3["litlen"] if l) == [8] * 256 and not any(b3["dist"])
    # HCLEN = 4: the one header it can spell has no end code
    with pytest.raises(ValueError, match="no end code"):
        Reader(CASES["hclen-4-all-zero"].raw).run()


def test_empty_blocks_at_every_alignment():
    blocks = parsed("empty-blocks-alignments").blocks
    assert [b["type"] for b in blocks] == [1, 0, 0, 1, 2, 2, 1] * 8 + [0]
    assert [b["final"] for b in blocks] == [0] * 56 + [1]
    for k in range(8):
        b = blocks[7 * k:7 * k + 7]
        assert b[0]["bit"] % 8 == k and b[1]["bit"] % 8 == (k + 2) % 8
        assert len(b[0]["tokens"]) == k + 1 and not copies(b[0])
        assert b[1]["len"] == 0 and 0 < b[2]["len"] < 16
        assert not b[3]["tokens"] and not b[4]["tokens"]
        assert len(copies(b[5])) == 1
        length, dist = copies(b[6])[0]
        at = b[6]["out"]
        assert b[2]["out"] <= at - dist < b[2]["out"] + b[2]["len"]                            # its source begins in the stored bytes
    assert blocks[-1]["len"] == 0


def test_stored_65535_then_copies():
    b1, b2, b3 = parsed("stored-65535-then-copies").blocks
    assert (b1["type"], len(b1["tokens"])) == (1, 1) and (b2["type"], b2["len"]) == (0, 65535)
    assert copies(b3) == [(258, 32768), (258, 1), (3, 32768)]


def test_overlapping_and_dependent_copies():
    (b,) = parsed("overlapping-copies").blocks
    assert {(length, d) for d in range(1, 10) for length in (258, 3, 17)} <= set(copies(b))
    (b,) = parsed("dependent-copies").blocks
    # runs of copies in a row, each at the distance of the length before it
    runs, run, prev = [], 0, None
    for t in b["tokens"]:
        if t[3] and prev and t[4] == prev:
            run += 1
        else:
            runs.append(run)
            run = 0
        prev = t[3] or None
    assert sorted(runs)[-2:] == [63, 199]
    cp = set(copies(b))
    assert {(length, length + k) for length in (47, 48, 49, 255, 256, 257, 258) for k in (-1, 0, 1)} <= cp
    # a source that straddles what is in place: it begins before the copy in front of it and ends inside it
    toks = b["tokens"]
    assert sum(1 for p, t in zip(toks, toks[1:]) if p[3] and t[3] and p[3] < t[4] < p[3] + t[3]) >= 40


def test_empty_text_and_only_end_code():
    blocks = parsed("empty-text-64").blocks
    assert len(blocks) >= 14 and all(b["type"] == 0 and b["len"] == 0 for b in blocks)
    assert len(CASES["empty-text-64"].member()) >= 64 and CASES["empty-text-64"].want == b""
    b = parsed("only-end-code").blocks[-1]
    assert [(s, l) for s, l in enumerate(b["litlen"]) if l] == [(256, 1)] and not b["tokens"]


def test_many_chunks():
    c = CASES["many-chunks"]
    r = parsed("many-chunks")
    assert 680 << 10 <= len(c.raw) <= 760 << 10 and len(c.want) < 32_000_000
    assert all(b["type"] == 2 and not b["final"] and complete(b["cl_lengths"]) and complete(b["litlen"]) and complete(b["dist"])
               for b in r.blocks[:-1])
    assert r.blocks[-1]["type"] == 0 and r.blocks[-1]["final"]
    # a block start in every territory of 16 KiB of the file: more than 40 chunks
    terr = {(80 + b["bit"]) // (16384 * 8) for b in r.blocks[:-1]}
    assert terr == set(range(len(c.member()) // 16384 + 1)) and len(terr) > 40
    lit = [t for b in r.blocks for t in b["tokens"]][:32768]
    assert all(not t[3] for t in lit) and sum(t[1] > 10 for t in lit) > 30000                   # 32 KiB of literals with long codes
    later = [b for b in r.blocks[:-1] if b["out"] >= 32768]
    assert {d for b in later for _, d in copies(b)} == {32768, 32767, 258, 1}
    assert all(sum(length for length, _ in copies(b)) > 0.99 * sum(t[3] or 1 for t in b["tokens"]) for b in later)


# ---------------------------------------------------------------------------------------------- k_gz_find's sieves, restated
def block_search(blob, terr_bytes, first_bit=80):
    """What gz_gpu.hpp's k_gz_find finds without `verify`: for every territory t >= 1 of the file the first bit position at
    which (1) a non-final dynamic block's header begins with counts of at most 286 and 30, (2) the code-length code's Kraft sum
    is exactly one, (3) all three codes are complete and there is an end code.  -> {t: bit position}"""
    bits = np.unpackbits(np.frombuffer(blob + bytes(64), dtype=np.uint8), bitorder="little").astype(np.int64)
    n = len(blob) * 8

    def field(p, off, width):
        return sum(bits[p + off + i] << i for i in range(width))
    p = np.arange(n)
    cand = p[(field(p, 0, 3) == 4) & (field(p, 3, 5) <= 29) & (field(p, 8, 5) <= 29)]
    ncl = field(cand, 13, 4) + 4
    ksum = np.zeros(len(cand), dtype=np.int64)
    for i in range(19):
        l = field(cand, 17 + 3 * i, 3)
        ksum += np.where((i < ncl) & (l > 0), 128 >> l, 0)
    cand = cand[ksum == 128]
    found = {}
    for q in map(int, cand):
        t = q // (terr_bytes * 8)
        if t == 0 or t in found or q <= first_bit:
            continue
        rd = Reader(blob)
        rd.pos = q
        try:
            blk = rd.block(header_only=True)
        except ValueError:
            continue
        if complete(blk["cl_lengths"]) and complete(blk["litlen"]) and complete(blk["dist"]):
            found[t] = q
    return found


def test_decoy_in_stored_is_a_false_start_for_the_block_search():
    c = CASES["decoy-in-stored"]
    r = parsed("decoy-in-stored")
    blob = c.member()
    assert len(blob) > 4 * 16384 + 16384
    kinds = [b["type"] for b in r.blocks[:-1]]
    assert set(kinds) == {0, 2} and kinds.count(0) == 3
    decoy = c.info["decoy"]
    d = Reader(decoy).block()
    assert d["type"] == 2 and not d["final"] and complete(d["cl_lengths"]) and complete(d["litlen"]) and complete(d["dist"])
    for b in r.blocks:
        if b["type"] == 0 and b["len"]:
            payload = c.raw[b["data"]:b["data"] + b["len"]]
            assert payload == (decoy * (len(payload) // len(decoy) + 1))[:len(payload)] and len(payload) > 3 * len(decoy)
    starts = {80 + b["bit"] for b in r.blocks}
    found = block_search(blob, 16384)
    assert sorted(found) == [1, 2, 3, 4, 5]
    false = [t for t, q in found.items() if q not in starts]
    assert false == [1, 3, 5]                                                                 # (at most eight are repaired)
    for t in false:
        q = found[t] - 80
        inside = [b for b in r.blocks if b["type"] == 0 and b["data"] * 8 <= q < (b["data"] + b["len"]) * 8]
        assert inside and (q // 8 - inside[0]["data"]) % len(decoy) == 0 and q % 8 == 0          # a copy of the decoy, inside a payload
    assert block_search(blob, 131072) == {}


# ---------------------------------------------------------------------------------------------- the host decoders
def gunzip(path, capacity, chunk=0):
    from tagdigger_amd import _binding as B
    L = B.load()
    buf = (C.c_uint8 * max(1, capacity))()
    n = C.c_uint64(0)
    rc = L.td_gunzip_file(str(path).encode(), buf, capacity, chunk, C.byref(n))
    return rc, bytes(memoryview(buf)[:n.value])


SETTINGS = ["sequential", "parallel-3000", "parallel-65536", "pipeline-3000", "pipeline-65536"]


@pytest.mark.parametrize("name,setting", [(n, s) for n in CASES for s in SETTINGS + (["parallel-700"] if n in ("many-chunks", "decoy-in-stored") else [])])
def test_gzip_member_through_the_host_decoders(tmp_path, monkeypatch, name, setting):
    """The five decoder settings of tests/test_inflate.py: fast_inflate.hpp, par_inflate.hpp in batches with chunks so small that
    most hold no block start, and the pipeline form that td_count_file drives."""
    monkeypatch.delenv("TAGDIG_ZLIB", raising=False)
    monkeypatch.delenv("TAGDIG_GUNZIP_PIPELINE", raising=False)
    if setting.startswith("pipeline"):
        monkeypatch.setenv("TAGDIG_GUNZIP_PIPELINE", "1")
    if setting == "sequential":
        monkeypatch.setenv("TAGDIG_PAR_INFLATE", "0")
    else:
        monkeypatch.setenv("TAGDIG_PAR_INFLATE", "1")
        monkeypatch.setenv("TAGDIG_INFLATE_CHUNK", setting.split("-")[1])
        monkeypatch.setenv("TAGDIG_INFLATE_THREADS", "4")
    c = CASES[name]
    p = tmp_path / "x.fq.gz"
    p.write_bytes(c.member())
    rc, got = gunzip(p, len(c.trailer_text) + 1000)
    if c.want is None:
        assert rc != 0
    else:
        assert rc == 0 and got == c.want


def zlib_produced(raw):
    """how many bytes zlib had produced when it refused the stream (fed byte by byte: what a call returns before the one
    that fails)"""
    d = zlib.decompressobj(-15)
    n = 0
    try:
        for i in range(len(raw)):
            n += len(d.decompress(raw[i:i + 1]))
    except zlib.error:
        return n
    raise AssertionError("zlib reads the stream")


@pytest.mark.parametrize("name", SMALL)
def test_lane_decoder_on_the_host(name):
    """gpu_inflate.hpp through td_inflate_raw_host: the decoder the GPU runs one BGZF member per lane."""
    from tagdigger_amd import _binding as B
    L = B.load()
    c = CASES[name]

    def inflate(n):
        out = (C.c_char * max(1, n + 8))()
        return L.td_inflate_raw_host(c.raw, len(c.raw), out, n), bytes(out[:n])
    if c.want is not None:
        assert inflate(len(c.want)) == (0, c.want)
        assert inflate(len(c.want) + 1)[0] != 0
        if c.want:
            assert inflate(len(c.want) - 1)[0] != 0
        return
    produced = zlib_produced(c.raw)
    assert inflate(produced)[0] != 0 and inflate(produced + 100)[0] != 0
    # ... and with the size of the text a decoder without the check would give: the size must not be what refuses the stream
    if c.lenient is not None:
        assert inflate(len(c.lenient))[0] != 0


def test_which_cases_the_lane_decoder_takes():
    assert set(CASES) - set(SMALL) == {"long-codes-max-tokens", "stored-65535-then-copies", "many-chunks", "decoy-in-stored"}
