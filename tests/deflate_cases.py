"""A DEFLATE writer from RFC 1951 and a catalogue of streams that no zlib encoder writes (tests/test_deflate_edges.py,
tests/test_deflate_edges_gpu.py): 15-bit literal/length codes next to 15-bit distance codes, length 258 as symbol 284
with 31 extra bits, the single 1-bit distance code, code-length repeats across the literal/distance boundary, empty blocks
of the three kinds at every bit alignment, chains of dependent and overlapping copies, real false block starts inside stored
blocks -- and the streams zlib refuses.  Other writers (libdeflate, igzip, zopfli, 7-Zip) emit such forms, and gzip.open
reads their files.

The writer knows nothing of the decoders under test: it writes what it is told to, and raises where it cannot (a token
whose symbol has no code), so that no case degrades silently; test_deflate_edges.py holds the catalogue against
zlib.decompress(raw, -15) and parses every stream again with a reader of its own.

A token is a literal (an int), a copy (length, distance) -- (258, distance, True) spells the length as symbol 284 with 31
extra bits --, or Raw(...) for symbols RFC 1951 does not define."""
import bisect
import struct
import zlib
from collections import Counter, namedtuple

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
GZIP_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"
WINDOW = 32768

# a literal/length symbol written as it is (with `lext` bits of `lval` behind it), then -- where dist_sym is not None --
# a distance symbol with `dext` bits of `dval`: for the symbols and combinations RFC 1951 leaves undefined
Raw = namedtuple("Raw", "litlen lext lval dist_sym dext dval", defaults=(0, 0, None, 0, 0))


def length_symbol(length, long258=False):
    """-> (symbol, extra bits, their value)"""
    if long258:
        assert length == 258
        return 284, 5, 31
    assert 3 <= length <= 258
    i = bisect.bisect_right(LENGTH_BASE, length) - 1
    return 257 + i, LENGTH_EXTRA[i], length - LENGTH_BASE[i]


def distance_symbol(dist):
    assert 1 <= dist <= 32768
    i = bisect.bisect_right(DIST_BASE, dist) - 1
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def _reverse(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical_codes(lengths):
    """RFC 1951 3.2.2: the codes of these lengths, each reversed once (DEFLATE packs Huffman codes from their most significant
    bit); None where the length is 0.  Nothing is checked: an over-subscribed set gives codes cut to their lengths."""
    count = Counter(l for l in lengths if l)
    code, nxt = 0, {}
    for bits in range(1, max(count, default=0) + 1):
        code = (code + count.get(bits - 1, 0)) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        if not l:
            out.append(None)
            continue
        out.append(_reverse(nxt[l] & ((1 << l) - 1), l))
        nxt[l] += 1
    return out


def kraft(lengths):
    """sum of 2^-l in units of 2^-15: 32768 is a complete code"""
    return sum(1 << (15 - l) for l in lengths if l)


def ladder(n, steps):
    """n code lengths of a complete code, ascending: 1, 2, ..., steps, and the other n - steps symbols share what is left
    as evenly as it goes.  ladder(16, 14) is 1 ... 14, 15, 15."""
    m = n - steps
    assert m >= 2
    j = m.bit_length() - 1
    short = (2 << j) - m                          # (all of them where m is a power of two)
    out = list(range(1, steps + 1)) + [steps + j] * short + [steps + j + 1] * (m - short)
    assert len(out) == n and max(out) <= 15 and kraft(out) == 32768, (n, steps, out)
    return out


def ladder_lengths(symbols, nsyms, steps):
    """`nsyms` lengths: ladder(len(symbols), steps) dealt to `symbols` in their order, 0 elsewhere"""
    out = [0] * nsyms
    for s, l in zip(symbols, ladder(len(symbols), steps)):
        out[s] = l
    return out


def by_frequency(data, rare_first=False):
    c = Counter(data)
    return sorted(c, key=lambda s: (c[s], s) if rare_first else (-c[s], s))


def rle_lengths(seq):
    """The code-length sequence of `seq` with symbols 16, 17 and 18, greedily (runs are taken across the literal/distance
    boundary where they happen to lie across it): ints for lengths, (16 | 17 | 18, count) for repeats."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k))
                run -= k
            if run >= 3:
                out.append((17, run))
                run = 0
            out += [0] * run
        else:
            out.append(v)
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k))
                run -= k
            out += [v] * run
        i = j
    return out


def spell_lengths(cl_symbols):
    """what a code-length sequence says (the reverse of rle_lengths); a 16 with nothing before it raises"""
    out = []
    for s in cl_symbols:
        if isinstance(s, int):
            out.append(s)
        elif s[0] == 16:
            out += [out[-1]] * s[1]
        else:
            out += [0] * s[1]
    return out


class DeflateWriter:
    """Bits, least significant first, and the three kinds of block.  `marks` gets (bit offset, size in bits, token) of every
    token written by fixed_block / dynamic_block; `blocks` (bit offset, type) of every block."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.marks = []
        self.blocks = []
        self.ntokens = 0

    @property
    def bitpos(self):
        return len(self.out) * 8 + self.n

    def bits(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def align(self):
        self.bits(0, -self.bitpos % 8)
        k = self.n >> 3
        self.out += self.acc.to_bytes(k, "little")
        self.acc, self.n = 0, 0

    def getvalue(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) >> 3, "little")

    # ------------------------------------------------------------ blocks
    def stored_block(self, final, data, len_field=None, nlen_field=None):
        assert len(data) <= 65535
        self.blocks.append((self.bitpos, 0))
        self.bits(final, 1)
        self.bits(0, 2)
        self.align()
        ln = len(data) if len_field is None else len_field
        self.out += struct.pack("<HH", ln, (ln ^ 0xFFFF) if nlen_field is None else nlen_field)
        self.out += data
        self.ntokens += len(data)                      # (the wave decoder makes a token of every stored byte)

    def fixed_block(self, final, tokens):
        self.blocks.append((self.bitpos, 1))
        self.bits(final, 1)
        self.bits(1, 2)
        self._tokens(tokens, FIXED_LITLEN, FIXED_DIST, True)

    def block_type_3(self, final):
        self.blocks.append((self.bitpos, 3))
        self.bits(final, 1)
        self.bits(3, 2)

    def dynamic_block(self, final, tokens, litlen_lengths, dist_lengths, cl_symbols=None, hclen=19, cl_lengths=None, end=True,
                      check=True):
        """cl_symbols: the code-length sequence spelled out -- ints for lengths 0 ... 15, (16, n) / (17, n) / (18, n) for the
        repeats with their counts; it must spell litlen_lengths + dist_lengths (check=False: whatever it spells).
        hclen: how many lengths of the code-length code are written (4 ... 19).  cl_lengths: that code's 19 lengths, where the
        balanced complete code this writer chooses will not do."""
        hlit, hdist = len(litlen_lengths) - 257, len(dist_lengths) - 1
        assert 0 <= hlit < 32 and 0 <= hdist < 32 and 4 <= hclen <= 19
        seq = list(litlen_lengths) + list(dist_lengths)
        if cl_symbols is None:
            cl_symbols = rle_lengths(seq)
        if check:
            assert spell_lengths(cl_symbols) == seq, "the code-length sequence does not spell the lengths"
        for s in cl_symbols:
            if not isinstance(s, int):
                lo, hi = {16: (3, 6), 17: (3, 10), 18: (11, 138)}[s[0]]
                assert lo <= s[1] <= hi, s
        if cl_lengths is None:
            used = by_frequency([s if isinstance(s, int) else s[0] for s in cl_symbols])
            for filler in CL_ORDER:                    # (the code-length code must be complete: two symbols at the least)
                if len(used) >= 2:
                    break
                if filler not in used:
                    used.append(filler)
            j = len(used).bit_length() - 1
            short = (2 << j) - len(used)
            cl_lengths = [0] * 19
            for k, s in enumerate(used):
                cl_lengths[s] = j if k < short else j + 1
        for s in range(19):
            if cl_lengths[s] and CL_ORDER.index(s) >= hclen:
                raise ValueError("HCLEN = %d does not reach code-length symbol %d" % (hclen, s))
        cl_codes = canonical_codes(cl_lengths)
        self.blocks.append((self.bitpos, 2))
        self.bits(final, 1)
        self.bits(2, 2)
        self.bits(hlit, 5)
        self.bits(hdist, 5)
        self.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.bits(cl_lengths[s], 3)
        for s in cl_symbols:
            sym = s if isinstance(s, int) else s[0]
            if cl_codes[sym] is None:
                raise ValueError("code-length symbol %d has no code" % sym)
            self.bits(cl_codes[sym], cl_lengths[sym])
            if sym == 16:
                self.bits(s[1] - 3, 2)
            elif sym == 17:
                self.bits(s[1] - 3, 3)
            elif sym == 18:
                self.bits(s[1] - 11, 7)
        self._tokens(tokens, list(litlen_lengths) + [0] * (288 - len(litlen_lengths)), list(dist_lengths) + [0] * (32 - len(dist_lengths)), end)

    def _tokens(self, tokens, llens, dlens, end):
        lcodes, dcodes = canonical_codes(llens), canonical_codes(dlens)
        cache = {}
        marks, bits = self.marks, self.bits
        for t in tokens:
            e = cache.get(t)
            if e is None:
                # the whole token as one value: code, extra bits, code, extra bits
                if isinstance(t, int):
                    fields = [(lcodes[t], llens[t])]
                elif isinstance(t, Raw):
                    fields = [(lcodes[t.litlen], llens[t.litlen]), (t.lval, t.lext)]
                    if t.dist_sym is not None:
                        fields += [(dcodes[t.dist_sym], dlens[t.dist_sym]), (t.dval, t.dext)]
                else:
                    ls, le, lv = length_symbol(t[0], len(t) > 2 and t[2])
                    ds, de, dv = distance_symbol(t[1])
                    fields = [(lcodes[ls], llens[ls]), (lv, le), (dcodes[ds], dlens[ds]), (dv, de)]
                v = nb = 0
                for val, n in fields:
                    if val is None:
                        raise ValueError("token %r needs a symbol that has no code" % (t,))
                    v |= val << nb
                    nb += n
                e = cache[t] = (v, nb)
            marks.append((len(self.out) * 8 + self.n, e[1], t))
            bits(e[0], e[1])
        self.ntokens += len(tokens)
        if end and llens[256]:
            self.bits(lcodes[256], llens[256])


def expand(tokens, history=b""):
    """the text of `tokens` behind `history`; a copy that reaches before the history raises ValueError"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        length, dist = t[0], t[1]
        s = len(out) - dist
        if s < 0:
            raise ValueError("distance too far back")
        if dist >= length:
            out += out[s:s + length]
        else:
            out += (bytes(out[s:]) * (length // dist + 1))[:length]
    return bytes(out[len(history):])


def member(raw, text):
    """one gzip member (its header is 10 bytes: a token at bit b of `raw` is at bit 80 + b of the file)"""
    return GZIP_HEADER + raw + struct.pack("<II", zlib.crc32(text), len(text) & 0xFFFFFFFF)


def bgzf_member(raw, text):
    total = 18 + len(raw) + 8
    assert total <= 65536 and len(text) <= 65536
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1)
            + raw + struct.pack("<II", zlib.crc32(text), len(text)))


def bgzf_file(members):
    return b"".join(members) + bgzf_member(b"\x03\x00", b"")


# ---------------------------------------------------------------------------------------------- the catalogue
class Case:
    """raw: the DEFLATE stream.  want: its text, or None where zlib refuses it.  device: the wave decoder (gz_gpu.hpp) must
    decode it itself (it may leave a valid file to the host only below 64 bytes, for an incomplete literal/length code, for a
    chunk with more tokens than 4 * span + 4096, for small members, or without room on the card); `why` names the reason
    where it need not.  ntokens: its tokens, a stored byte counting as one.  lenient: for a refused stream, the text a decoder
    gives that lacks the one check the case is about (what the member's trailer is written for, so that the CRC-32 and the
    length cannot be what refuses it).  info: what the case claims about its own structure."""

    def __init__(self, name, writer, want, device=True, why="", lenient=None, **info):
        self.name, self.raw, self.want, self.device, self.why = name, writer.getvalue(), want, device, why
        self.ntokens, self.marks, self.blocks, self.lenient, self.info = writer.ntokens, writer.marks, writer.blocks, lenient, info
        self.trailer_text = want if want is not None else (lenient or b"")

    def member(self):
        return member(self.raw, self.trailer_text)

    def __repr__(self):
        return "Case(%s)" % self.name


_CACHE = {}


def synth_config():
    if "cfg" not in _CACHE:
        from tagdigger_amd.synth import SynthConfig
        _CACHE["cfg"] = SynthConfig.from_id(1, nreads=4000)
    return _CACHE["cfg"]


def reads(n=None):
    """the first reads of the synthetic library (219 bytes each): literals that count"""
    if "reads" not in _CACHE:
        from helpers import synth_host_bytes
        cfg = synth_config()
        _CACHE["reads"] = synth_host_bytes(cfg, 0, cfg.nreads).tobytes()
    rb = synth_config().record_bytes
    return _CACHE["reads"] if n is None else _CACHE["reads"][:n * rb]


def step_lanes(marks, first, last):
    """The lane each token of marks[first:last] (one block's) starts at in the wave decoder's steps: a step looks at the 64 bit
    positions from where the step before ended, and ends behind the last token that starts in them.  -> [(lane, the step's first
    bit), ...]"""
    out, step = [], marks[first][0]
    for at, _, _ in marks[first:last]:
        if at - step >= 64:
            step = at
        out.append((at - step, step))
    return out


def _text_code(data, extra, steps, rare_first=False):
    """286 literal/length lengths: a ladder over the bytes of `data` by frequency, then `extra` (the longest codes)"""
    syms = by_frequency(data, rare_first) + list(extra)
    return ladder_lengths(syms, 286, min(steps, len(syms) - 2))


def _preamble(w, nreads=1):
    """short cases: a fixed block of literals in front, so that the file has its 64 bytes and the counts are not zero"""
    text = reads(nreads)
    w.fixed_block(0, list(text))
    return text


def _long_codes(name, ncycles, length_symbols):
    """15-bit literal/length codes next to the 15-bit distance code 29 with its 13 extra bits.  Block 1 is as the catalogue's
    description has it: lengths 1 ... 14, 15, 15 over fourteen literals, 256 and 285 (its tokens are at most 15 + 0 + 15 + 13 = 43
    bits); block 2 gives 285's place to 284, so that (258, d) is 15 + 5 + 15 + 13 = 48 bits, the longest token there is.  In both,
    a pad of x bits of literals (14-bit ones and one shorter) in front of each copy, x = 0 ... 63, puts the copies at every
    lane of a step and every bit offset of a word."""
    table = bytes.maketrans(b"456789", b"000000")
    pre = reads(152).translate(table)
    order = [s for s in by_frequency(pre) if s != ord("N")] + [ord("N")]
    assert len(order) == 14, order
    dist = [0] * 30
    for i in range(14):
        dist[i] = i + 1
    dist[14] = dist[29] = 15
    w = DeflateWriter()
    tokens_all, spans = [], []
    for blk, lsym in enumerate(length_symbols):
        litlen = [0] * 286
        for i, s in enumerate(order):
            litlen[s] = i + 1
        litlen[256] = litlen[lsym] = 15
        assert sum(litlen[b] <= 10 for b in pre) >= WINDOW        # 32 KiB of short-code literals come first
        assert sorted(l for l in litlen if l) == ladder(16, 14) and sorted(l for l in dist if l) == ladder(16, 14)
        by_len = {litlen[s]: s for s in order}
        tokens = list(pre) if blk == 0 else []
        size = 43 if lsym == 285 else 48
        for cyc in range(ncycles):
            for x in range(64):
                d = 32768 if x == 0 else 24577 if x == 1 else 24577 + (x * 131 + cyc * 1777 + blk * 4099) % 8192
                copy = (258, d) if lsym == 285 else (258, d, True)
                tokens += [by_len[14]] * (x // 14) + ([by_len[x % 14]] if x % 14 else []) + [copy]
                if x + size < 64:
                    tokens.append(copy)           # (the next pad starts a step of its own)
        first = len(w.marks)
        w.dynamic_block(int(blk == len(length_symbols) - 1), tokens, litlen, dist)
        spans.append((first, len(w.marks)))
        tokens_all += tokens
    text = expand(tokens_all)
    # what the case is for, asserted where it is built
    big = [(at, nb) for at, nb, t in w.marks if not isinstance(t, int)]
    assert {nb for _, nb in big} == {43 if l == 285 else 48 for l in length_symbols}
    five = [at for at, nb in big if nb == 48 and 1985 <= (80 + at) % 2048 <= 2047]
    if ncycles > 1:                               # (the small form, for the decoders of members up to 64 KiB, has one round of pads)
        for size in {nb for _, nb in big}:
            assert {at % 64 for at, nb in big if nb == size} == set(range(64)), "token offsets modulo 64"
        for first, last in spans:
            lanes = {lane for (lane, _), (_, _, t) in zip(step_lanes(w.marks, first, last), w.marks[first:last]) if not isinstance(t, int)}
            assert lanes == set(range(64)), "a copy at every lane of a step"
        assert five, "no 48-bit token starts in the last 63 bits of a 2048-bit block of the file"
    return Case(name, w, text, ncopies=len(big), five_word_tokens=len(five))


def _c_long258():
    w = DeflateWriter()
    pre = reads(1)
    tokens = list(pre) + [(258, 219, True), (258, 1, True), ord("\n"), (258, 300, True), (258, 258, True), (258, 2, True), ord("\n")]
    w.fixed_block(1, tokens)
    return Case("258-as-284-31", w, expand(tokens))


def _c_dist_exact():
    w = DeflateWriter()
    pre = reads(150)[:WINDOW]
    w.dynamic_block(0, list(pre), _text_code(pre, [256], 8), [0])
    tokens = [(258, 32768), (3, 32768), (258, 32768)]            # the first one's source begins at byte 0 of the member
    w.fixed_block(1, tokens)
    return Case("dist-32768-exact", w, pre + expand(tokens, pre))


def _c_one_distance_code():
    w = DeflateWriter()
    pre = reads(2)
    tokens = list(pre) + [(258, 1), ord("\n"), (3, 1), (17, 1), ord("\n")]
    litlen = _text_code(pre, [256] + sorted({length_symbol(t[0])[0] for t in tokens if not isinstance(t, int)}), 6)
    w.dynamic_block(1, tokens, litlen, [1])                       # HDIST = 1 (the field is 0): one code of one bit, and it is used
    return Case("one-distance-code", w, expand(tokens))


def _c_no_distance_code():
    w = DeflateWriter()
    pre = reads(2)
    w.dynamic_block(1, list(pre), _text_code(pre, [256], 6), [0])
    return Case("no-distance-code", w, pre)


def _c_repeat_across():
    """Block 1: HLIT = 258 lengths and a symbol 16 whose run covers the last literal/length length and the first distance
    lengths.  Block 2: HLIT = 286, symbol 285 used, 18-runs of 138.  Block 3: HCLEN = 5.  (HCLEN = 4 reaches the symbols 16,
    17, 18 and 0 only: every length is 0, there is no end code, no valid header exists -- the catalogue has that header among
    the refused streams; 5 adds the length 8: 256 codes of 8 bits, literals only.)"""
    w = DeflateWriter()
    text = reads(3)
    a, b, c = text[:219], text[219:438], text[438:]
    # block 1: the literals by a ladder whose last place is split in four, for 256, 257 and two literals nothing uses: `tail` bits
    lits = by_frequency(a)
    lad = ladder(len(lits) + 1, 3)
    tail = lad[-1] + 2
    litlen = [0] * 258
    for s, l in zip(lits, lad):
        litlen[s] = l
    for s in [s for s in range(250, 256) if not litlen[s]][:2] + [256, 257]:
        litlen[s] = tail
    assert kraft(litlen) == 32768
    # a complete distance code whose first six lengths are `tail` too: what they leave, in shorter codes behind them
    dist = [tail] * 6
    room = 32768 - kraft(dist)
    for l in range(1, 16):
        if room & (1 << (15 - l)):
            dist.append(l)
    assert kraft(dist) == 32768 and len(dist) <= 30
    cl = rle_lengths(litlen[:256]) + [tail, (16, 6), tail] + dist[6:]      # 256 | 257 and five distances by ONE repeat | the sixth
    tokens = list(a) + [(3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (3, 6), ord("\n")]
    w.dynamic_block(0, tokens, litlen, dist, cl_symbols=cl, hclen=19)
    t1 = expand(tokens)
    # block 2: HLIT = 286, 285 in use, the zeros between the literals and 256 by an 18-run of 138
    litlen2 = _text_code(b, [256, 285], 6)
    dist2 = [0] * 15 + [1]                                        # one distance code of one bit: number 15 (193 ... 256)
    cl2 = rle_lengths(litlen2 + dist2)
    assert (18, 138) in cl2 and len(litlen2) == 286
    tokens2 = list(b) + [(258, 219), ord("\n")]
    w.dynamic_block(0, tokens2, litlen2, dist2, cl_symbols=cl2, hclen=19)
    t2 = expand(tokens2, t1)
    # block 3: 256 codes of 8 bits -- 0 ... 254 and 256 --, no distance code, HCLEN = 5 (16, 17, 18, 0, 8)
    litlen3 = [8] * 255 + [0, 8]
    cl3 = [8, (16, 6)] * 36 + [8, 8, 8, 0, 8, 0]
    cl_lengths = [0] * 19
    cl_lengths[8], cl_lengths[16], cl_lengths[0] = 1, 2, 2
    w.dynamic_block(1, list(c), litlen3, [0], cl_symbols=cl3, hclen=5, cl_lengths=cl_lengths)
    return Case("repeat-across-lit-dist", w, t1 + t2 + c, hlit=(258, 286, 257), hclen=(19, 19, 5))


EMPTY_DYNAMIC = dict(litlen_lengths=[0] * 65 + [1] + [0] * 190 + [1], dist_lengths=[0])      # 'A' and the end code, one bit each


def _c_empty_blocks():
    w = DeflateWriter()
    text = bytearray()
    src = reads(8)
    at = 0
    for k in range(8):
        # iteration k begins at bit alignment k (and its empty stored block at k + 2 + 8 (k + 1)): short copies of 12 ... 15
        # bits at the end of the block before shift the alignment
        assert w.bitpos % 8 == k, (k, w.bitpos)
        t1 = list(src[at:at + k + 1])
        at += k + 1
        w.fixed_block(0, t1)
        text += bytes(t1)
        w.stored_block(0, b"")
        st = src[at:at + 5 + k]
        at += 5 + k
        w.stored_block(0, st)
        text += st
        w.fixed_block(0, [])
        w.dynamic_block(0, [], **EMPTY_DYNAMIC)
        t6 = list(src[at:at + 20]) + [(4 + k, 3 + k)]
        at += 20
        w.dynamic_block(0, t6, _text_code(src[at - 20:at], [256, length_symbol(4 + k)[0]], 3), [0] * distance_symbol(3 + k)[0] + [1])
        text += expand(t6, bytes(text))
        t7 = [(3 + k, 27 + k), ord("\n")]                           # its source: the last 3 stored bytes and the first of block 6
        # alignment for the next iteration: the bits of this block are 3 + tokens + 7
        probe = DeflateWriter()
        probe.bits(0, w.bitpos % 8)
        probe.fixed_block(0, t7)
        a, b, c, d = (3, 1), (3, 5), (3, 9), (3, 17)                # 7 + 5 bits and 0, 1, 2, 3 extra bits of distance
        t7 += [[], [b, a], [b, b], [b, c], [a], [b], [c], [d]][(k + 1 - probe.bitpos) % 8]
        w.fixed_block(0, t7)
        text += expand(t7, bytes(text))
    w.stored_block(1, b"")
    return Case("empty-blocks-alignments", w, bytes(text))


def _c_stored_65535():
    w = DeflateWriter()
    w.fixed_block(0, [ord("@")])
    body = reads(300)[1:65536]
    w.stored_block(0, body)
    tokens = [(258, 32768), (258, 1), (3, 32768), ord("\n")]
    w.fixed_block(1, tokens)
    pre = b"@" + body
    return Case("stored-65535-then-copies", w, pre + expand(tokens, pre))


def _c_overlapping():
    w = DeflateWriter()
    pre = reads(1)
    tokens = list(pre)
    for d in range(1, 10):
        for length in (258, 3, 17):
            tokens += [(length, d), ord("ACGT"[d % 4])]
        tokens.append(ord("\n"))
    w.fixed_block(1, tokens)
    return Case("overlapping-copies", w, expand(tokens))


def _c_dependent():
    """k_gz_lz makes the copies of 64 tokens in rounds: a copy waits for the copies in front of it that it reads from."""
    w = DeflateWriter()
    pre = reads(3)
    tokens = list(pre)
    # 64 and then 200 copies in a row, each reading what the one before wrote (the distance is the length before)
    for n, seed in ((64, 5), (200, 11)):
        prev = 219
        for i in range(n):
            length = 3 + (i * seed * 7 + i * i) % 120
            tokens.append((length, prev))
            prev = length
        tokens += [ord("\n"), ord("@")]
    # copies whose source straddles the end of what is in place: part of it from before the run, part from the copy in front
    for i in range(40):
        tokens.append((30 + i, 30 + i - 1 + 7))                   # reads 7 bytes from before the copy in front of it, the rest from it
        tokens.append((9 + i % 5, 4 + i % 7))
    tokens.append(ord("\n"))
    # the cooperative path's edges: L >= 48, L <= dist, and its rest of L mod 4 symbols
    for length in (47, 48, 49, 255, 256, 257, 258):
        for dist in (length, length - 1, length + 1):
            tokens += [(length, dist), ord("G")]
        tokens += [(length, length), (length, length), (length, length + 1)]       # ... and those as a chain
        tokens.append(ord("\n"))
    w.fixed_block(1, tokens)
    return Case("dependent-copies", w, expand(tokens))


def _c_empty_text():
    w = DeflateWriter()
    for _ in range(14):
        w.stored_block(0, b"")
    w.stored_block(1, b"")
    c = Case("empty-text-64", w, b"")
    assert len(c.member()) >= 64
    return c


def _c_only_end_code():
    w = DeflateWriter()
    pre = _preamble(w)
    w.dynamic_block(1, [], [0] * 256 + [1], [0])
    return Case("only-end-code", w, pre, device=False, why="a Huffman code this decoder leaves to zlib")


def _many_chunks_codes(sample, length_syms=(263, 273, 285), dist_syms=(0, 16, 29)):
    """One header for all blocks: the rare literals get the short codes, so that the frequent ones, the end code and the
    length symbols have 14 and 15 bits (codes longer than the decoder's 10-bit table index, nearly every token); the distance
    codes in use have 14 and 15 bits behind codes that nothing uses.  All three codes are complete."""
    lits = by_frequency(sample, rare_first=True)
    syms = lits + list(length_syms) + [256]
    litlen = ladder_lengths(syms, 286, len(syms) - 13)
    fill = [s for s in range(30) if s not in dist_syms][:16 - len(dist_syms)]
    dist = [0] * 30
    for s, l in zip(fill + list(dist_syms), ladder(16, 14)):
        dist[s] = l
    return litlen, dist


def _c_many_chunks():
    w = DeflateWriter()
    src = reads()
    litlen, dist = _many_chunks_codes(src)
    out = bytearray()
    rb = 219
    for i in range(0, 150, 30):                                  # the first 32 KiB: literals
        part = src[i * rb:(i + 30) * rb]
        w.dynamic_block(0, list(part), litlen, dist)
        out += part
    at = 150 * rb
    target = 700 << 10
    while len(w.out) < target:
        tokens = []
        for _ in range(100):
            tokens += [(258, 32768)] * 3 + [src[at], src[at + 1], (258, 32767), (37, 258), (9, 1), 10]
            at = (at + 2) % (len(src) - 2)
        w.dynamic_block(0, tokens, litlen, dist)
        out += expand(tokens, bytes(out[-WINDOW:]))
    w.stored_block(1, b"")
    text = bytes(out)
    assert len(text) < 32_000_000
    return Case("many-chunks", w, text, longest_line=max(map(len, text.split(b"\n"))))


def _c_decoy():
    """Stored blocks whose payload is a complete, valid, non-final dynamic block, over and over: the block search meets its
    header in the territories that begin inside such a payload -- a false start: the chunk in front of it runs past it, the
    host drops it and has the stretch decoded again.  Laid out for territories of 16 KiB of the FILE (10 bytes of header in
    front of the stream): the boundaries at 16, 48 and 80 KiB lie in stored payloads, those at 32 and 64 KiB in runs of small
    dynamic blocks.  The text stays FASTQ: the dynamic blocks hold whole records, and the decoy's bytes are chosen without a
    line end among them, so that a payload is the beginning of one long header line."""
    src = reads()
    rb = 219
    litlen, dist = _many_chunks_codes(src, length_syms=(283,), dist_syms=(15,))
    for k in range(3000):
        dw = DeflateWriter()
        dw.dynamic_block(0, list(src[k * rb:(k + 1) * rb]) + [(219, 219)], litlen, dist)
        decoy = dw.getvalue()
        if b"\n" not in decoy and b"\r" not in decoy:
            break
    else:
        raise AssertionError("no decoy without a line end")
    w = DeflateWriter()
    out = bytearray()
    at = 0

    def dynamic_run(until):                                      # small dynamic blocks until the file position `until`
        nonlocal at
        while 10 + len(w.out) < until:
            part = src[at:at + 2 * rb]
            at += 2 * rb
            tokens = list(part) + [(219, 219)]                   # (the third record: the second once more)
            w.dynamic_block(0, tokens, litlen, dist)
            out.extend(expand(tokens, bytes(out[-WINDOW:])))

    def stored_run(until):
        n = until - (10 + len(w.out)) - 5
        payload = (decoy * (n // len(decoy) + 1))[:n]
        w.stored_block(0, payload)
        out.extend(payload)

    for boundary in (16 << 10, 48 << 10, 80 << 10):
        dynamic_run(boundary - 1024)
        assert 10 + len(w.out) < boundary - 64
        stored_run(boundary + 2048)
    dynamic_run(90 << 10)
    w.stored_block(1, b"")
    text = bytes(out)
    return Case("decoy-in-stored", w, text, decoy=decoy, longest_line=max(map(len, text.split(b"\n"))))


# ------------------------------------------------------------------ refused by zlib
def _refused(name, build):
    w = DeflateWriter()
    pre = _preamble(w)
    extra = build(w, pre)
    return Case(name, w, None, lenient=(pre + extra) if extra is not None else None)


def _zero_window_text(tokens):
    return expand(tokens, bytes(WINDOW))


def _c_dist_too_far():
    w = DeflateWriter()
    pre = reads(150)[:WINDOW - 1]
    w.dynamic_block(0, list(pre), _text_code(pre, [256], 8), [0])
    tokens = [(258, 32768), ord("\n")]
    w.fixed_block(1, tokens)
    return Case("dist-too-far", w, None, lenient=pre + expand(tokens, bytes(1) + pre))


def _c_copy_from_nothing():
    w = DeflateWriter()
    tokens = [(20, 1)] + list(reads(1))
    w.fixed_block(1, tokens)
    return Case("copy-from-nothing", w, None, lenient=_zero_window_text(tokens))


def _c_toofar_zero_trailer():
    w = DeflateWriter()
    tokens = list(reads(1)) + [(258, 32768), (100, 300), ord("\n")] + list(reads(2)[219:])
    w.fixed_block(1, tokens)
    return Case("toofar-zero-trailer", w, None, lenient=_zero_window_text(tokens))


def _build_refused():
    a = reads(2)[219:]
    code = _text_code(a, [256], 6)

    def repeat_first(w, pre):
        cl = [(16, 3)] + rle_lengths(code[3:] + [0])
        w.dynamic_block(1, list(a), code, [0], cl_symbols=cl, check=False)

    def symbol_286(w, pre):
        w.fixed_block(1, list(a) + [Raw(286)] + list(a))

    def distance_30(w, pre):
        w.fixed_block(1, list(a) + [Raw(257, 0, 0, 30, 0, 0)] + list(a))

    def oversubscribed(w, pre):
        over = list(code)
        over[min(s for s in range(256) if not over[s])] = 1
        assert kraft(over) > 32768
        w.dynamic_block(1, list(a), over, [0])

    def incomplete(w, pre):
        # (every code the tokens use exists: only the header says that the stream is invalid)
        inc = list(code)
        longest = max(inc)
        drop = [s for s in range(256) if inc[s] == longest][0]
        inc[drop] = 0
        assert kraft(inc) < 32768 and sum(1 for l in inc if l) >= 2
        toks = [t for t in a if t != drop]
        w.dynamic_block(1, toks, inc, [0])
        return bytes(toks)

    def incomplete_distance(w, pre):
        toks = list(a) + [(5, 1), (6, 2), 10]
        lc = _text_code(a, [256, 259, 260], 6)
        w.dynamic_block(1, toks, lc, [2, 2])
        return expand(toks, pre)

    def incomplete_code_lengths(w, pre):
        cl_lengths = [0] * 19
        for sym in {x if isinstance(x, int) else x[0] for x in rle_lengths(code + [0])}:
            cl_lengths[sym] = 5                                   # (at most 19 codes of 5 bits: what is spelled is valid but for this)
        assert kraft(cl_lengths) < 32768
        w.dynamic_block(1, list(a), code, [0], cl_lengths=cl_lengths)
        return a

    def no_distance_defined(w, pre):
        lc = _text_code(a, [256, 259], 6)
        w.dynamic_block(1, list(a) + [Raw(259, 0, 0)] + list(a), lc, [0])

    def type_3(w, pre):
        w.block_type_3(1)

    def stored_nlen(w, pre):
        w.stored_block(1, a, nlen_field=(len(a) ^ 0xFFFF) ^ 0x0100)
        return a

    def hlit_287(w, pre):
        w.dynamic_block(1, list(a), code + [0], [0])

    def no_end_code(w, pre):
        ne = _text_code(a, [], 6)
        assert ne[256] == 0 and kraft(ne) == 32768
        w.dynamic_block(1, list(a), ne, [0])

    def hclen_4(w, pre):
        # the only header HCLEN = 4 can spell: every length 0 (symbols 16, 17, 18 and 0 are all it reaches)
        cl_lengths = [0] * 19
        cl_lengths[18] = cl_lengths[0] = 1
        w.dynamic_block(1, [], [0] * 257, [0], cl_symbols=[(18, 138), (18, 120)], hclen=4, cl_lengths=cl_lengths, end=False)

    table = [("repeat-with-no-previous", repeat_first), ("fixed-symbol-286", symbol_286), ("fixed-distance-30", distance_30),
             ("oversubscribed-litlen", oversubscribed), ("incomplete-litlen", incomplete), ("incomplete-distance", incomplete_distance),
             ("incomplete-code-length-code", incomplete_code_lengths),
             ("distance-used-but-none-defined", no_distance_defined), ("block-type-3", type_3), ("stored-len-nlen", stored_nlen),
             ("hlit-287", hlit_287), ("no-end-of-block-code", no_end_code), ("hclen-4-all-zero", hclen_4)]
    return [_refused(name, fn) for name, fn in table]


def catalogue():
    """name -> Case, built once"""
    if "cases" not in _CACHE:
        cases = [_long_codes("long-codes-max-tokens", 5, (285, 284)), _long_codes("long-codes-small", 1, (284,))]
        cases += [_c_long258(), _c_dist_exact(), _c_one_distance_code(), _c_no_distance_code(), _c_repeat_across(),
                  _c_empty_blocks(), _c_stored_65535(), _c_overlapping(), _c_dependent(), _c_empty_text(), _c_only_end_code(),
                  _c_many_chunks(), _c_decoy(), _c_dist_too_far(), _c_copy_from_nothing(), _c_toofar_zero_trailer()]
        cases += _build_refused()
        for c in cases:
            if c.want is not None and c.device:
                # the wave decoder's contract: such a file is its own
                assert len(c.member()) >= 64, c.name
                assert c.ntokens + 192 <= 4 * len(c.raw) + 4096, (c.name, c.ntokens, len(c.raw))
        _CACHE["cases"] = {c.name: c for c in cases}
        assert len(_CACHE["cases"]) == len(cases)
    return _CACHE["cases"]


def valid_names():
    return [n for n, c in catalogue().items() if c.want is not None]


def refused_names():
    return [n for n, c in catalogue().items() if c.want is None]
