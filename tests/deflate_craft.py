"""A DEFLATE (RFC 1951) writer for tests, and a plain inflate that reports what a stream contains.  Nothing here touches the library.

The writer optimises nothing: the caller decides every bit -- the code lengths of all three codes, how the sequence of lengths is spelled with 16 / 17 / 18,
HLIT, HDIST and HCLEN, and every token.  That is how the tests reach the valid shapes no zlib ever writes (a run across the literal/length | distance
boundary, a single one-bit distance code, length 258 as 284 + 31 ...) and the invalid ones.  The authority on bytes is always zlib.decompressobj(-15):
accepted(), below.  census() only describes a stream; it is restated from the RFC on its own and shares no table with the code under test."""
import zlib

# RFC 1951 section 3.2.5: length symbols 257..285 and distance symbols 0..29 (two unused slots behind each, so that an invalid symbol can be written)
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0] + [0, 0]
LBASE = []
for _i in range(28):
    LBASE.append(3 if _i == 0 else LBASE[-1] + (1 << LEXT[_i - 1]))
LBASE += [258, 0, 0]
DEXT = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)] + [0, 0]
DBASE = []
for _i in range(30):
    DBASE.append(1 if _i == 0 else DBASE[-1] + (1 << DEXT[_i - 1]))
DBASE += [0, 0]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
assert LBASE[:29] == [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258] and DBASE[29] == 24577 and DEXT[29] == 13


class BitWriter:
    """LSB first, as RFC 1951 packs everything but the Huffman codes themselves"""

    def __init__(self):
        self.buf = bytearray()
        self.nbits = 0

    def bits(self, v, k):
        for i in range(k):
            if self.nbits & 7 == 0:
                self.buf.append(0)
            self.buf[-1] |= ((v >> i) & 1) << (self.nbits & 7)
            self.nbits += 1

    def code(self, c):
        """a Huffman code (value, length): its most significant bit goes first"""
        v, k = c
        for i in range(k - 1, -1, -1):
            self.bits((v >> i) & 1, 1)

    def align(self):
        self.nbits = (self.nbits + 7) & ~7

    def raw(self, data):
        assert self.nbits & 7 == 0
        self.buf += data
        self.nbits += 8 * len(data)

    def getvalue(self):
        return bytes(self.buf)


def canonical(lengths):
    """[(code, length) or None per symbol]: the canonical code of RFC 1951 3.2.2 -- whatever the lengths are, complete or not"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append(None)
        else:
            out.append((nxt[l], l))
            nxt[l] += 1
    return out


def complete_lengths(symbols, n):
    """n code lengths, non-zero for `symbols` (two or more): a complete code with all codes as near one length as it goes -- a convenience, no Huffman construction"""
    k = len(symbols)
    assert k >= 2
    top = (k - 1).bit_length()
    short = (1 << top) - k
    lens = [0] * n
    for i, s in enumerate(sorted(symbols)):
        lens[s] = top - 1 if i < short else top
    return lens


def rle(seq, breaks=(), use16=True):
    """greedy spelling of a length sequence with 16 / 17 / 18: [(symbol, extra)].  No run crosses an index in `breaks` (zlib breaks at the table boundary;
    a single-sequence encoder passes breaks=()); use16=False spells repeated non-zero lengths one by one"""
    out, i, n = [], 0, len(seq)
    stops = sorted(set(breaks) | {n})
    while i < n:
        lim = min(s for s in stops if s > i)
        run = 1
        while i + run < lim and seq[i + run] == seq[i]:
            run += 1
        if seq[i] == 0 and run >= 3:
            r = min(run, 138)
            out.append((18, r - 11) if r >= 11 else (17, r - 3))
            i += r
            continue
        out.append((seq[i], 0))
        i += 1
        run -= 1
        while use16 and run >= 3:
            r = min(run, 6)
            out.append((16, r - 3))
            i += r
            run -= r
    return out


def expand(spelling):
    """the length sequence a spelling stands for (a 16 at the start repeats nothing: 0)"""
    out = []
    for s, x in spelling:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1] if out else 0] * (3 + x)
        elif s == 17:
            out += [0] * (3 + x)
        else:
            out += [0] * (11 + x)
    return out


def match(dist, length, alt258=False):
    """the token (length symbol, extra, distance symbol, extra) of a match; alt258 writes length 258 as symbol 284 with extra 31"""
    if length == 258:
        ls, lx = (284, 31) if alt258 else (285, 0)
    else:
        ls = max(s for s in range(28) if LBASE[s] <= length) + 257
        lx = length - LBASE[ls - 257]
    ds = max(s for s in range(30) if DBASE[s] <= dist)
    return (ls, lx, ds, dist - DBASE[ds])


class Stream:
    """one deflate stream in the making.  .out is the payload the tokens stand for, by the plain rule; .marks the bit offsets behind every token and every block.
    Tokens: an int 0..255 is a literal; (length symbol, extra, distance symbol, extra) a match (distance symbol None: the length half alone);
    ("bits", value, count) raw bits; ("sym", s) the literal/length code of symbol s alone."""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()
        self.marks = []
        self.impossible = False           # a token reached before the output start: .out is not meaningful

    def _header(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False, len_=None, nlen=None, body=None):
        self._header(final, 0)
        self.w.align()
        n = len(data) if len_ is None else len_
        self.w.bits(n, 16)
        self.w.bits((~n & 0xffff) if nlen is None else nlen, 16)
        self.w.raw(data if body is None else body)
        self.out += data
        self.marks.append(self.w.nbits)
        return self

    def _tokens(self, tokens, ll, d, eob):
        for t in tokens:
            if isinstance(t, int):
                self.w.code(ll[t])
                self.out.append(t)
            elif t[0] == "bits":
                self.w.bits(t[1], t[2])
            elif t[0] == "sym":
                self.w.code(ll[t[1]])
            else:
                ls, lx, ds, dx = t
                self.w.code(ll[ls])
                self.w.bits(lx, LEXT[ls - 257])
                if ds is not None:
                    self.w.code(d[ds])
                    self.w.bits(dx, DEXT[ds])
                    length, dist = LBASE[ls - 257] + lx, DBASE[ds] + dx
                    if dist == 0 or dist > len(self.out):
                        self.impossible = True
                    else:
                        for _ in range(length):
                            self.out.append(self.out[-dist])
            self.marks.append(self.w.nbits)
        if eob:
            self.w.code(ll[256])
        self.marks.append(self.w.nbits)

    def fixed(self, tokens, final=False, eob=True):
        self._header(final, 1)
        self._tokens(tokens, canonical(FIXED_LL), canonical(FIXED_D), eob)
        return self

    def dynamic(self, ll_lens, d_lens, tokens, final=False, cl_lens=None, spelling=None, hlit=None, hdist=None, hclen=None, eob=True):
        """ll_lens / d_lens: the code lengths sent (HLIT + 257 and HDIST + 1 of them unless hlit / hdist say otherwise); spelling: [(code-length symbol, extra)] for
        the two together, default one symbol per length; cl_lens: the 19 lengths of the code-length code by symbol, default complete_lengths over the symbols
        the spelling uses; hclen: how many of them are sent, default up to the last non-zero one in the order of the RFC"""
        self._header(final, 2)
        if spelling is None:
            spelling = [(l, 0) for l in list(ll_lens) + list(d_lens)]
        if cl_lens is None:
            used = {s for s, _ in spelling}
            cl_lens = complete_lengths(used | ({0, 8} if len(used) < 2 else set()), 19)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CLORDER) if cl_lens[s]])
        self.w.bits(len(ll_lens) - 257 if hlit is None else hlit, 5)
        self.w.bits(len(d_lens) - 1 if hdist is None else hdist, 5)
        self.w.bits(hclen - 4, 4)
        for s in CLORDER[:hclen]:
            self.w.bits(cl_lens[s], 3)
        cl = canonical(cl_lens)
        for s, x in spelling:
            self.w.code(cl[s])
            if s >= 16:
                self.w.bits(x, (2, 3, 7)[s - 16])
        self.marks.append(self.w.nbits)
        self._tokens(tokens, canonical(ll_lens), canonical(d_lens), eob)
        return self

    def getvalue(self):
        return self.w.getvalue()


def accepted(comp, isize):
    """the reference's verdict: zlib ends the stream (eof) with exactly isize bytes -> (verdict, bytes, unused_data)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(comp, isize + 1)
    except zlib.error:
        return False, b"", b""
    return d.eof and len(out) == isize, out, d.unused_data


# ---------------------------------------------------------------- the plain inflate and its census
class DeflateError(Exception):
    pass


def new_census():
    return dict(blocks=[0, 0, 0], max_ll_len=0, max_d_len=0, max_cl_len=0, ll_decoded=set(), d_decoded=set(), cl_decoded=set(),
                runs_across=set(), runs_end_at_boundary=set(), runs_start_at_boundary=set(), n_dist_codes=set(), lsyms={}, dsyms={},
                min_dist=None, max_dist=None, min_len=None, max_len=None, overlaps=set(), hlit=set(), hdist=set(), hclen=set(), trailing=0,
                stored_after_bit=set(), back_over_block=0, back_into_stored=0, match_at={}, final_block=None, ll_code_sizes=set())


def _table(lengths):
    """(lookup by the next maxlen bits -> (symbol, length) or None, maxlen)"""
    mx = max(lengths) if lengths else 0
    if mx == 0:
        return [None], 0
    tab = [None] * (1 << mx)
    for s, c in enumerate(canonical(lengths)):
        if c is None:
            continue
        v, l = c
        r = int(format(v, "0%db" % l)[::-1], 2)
        if r < (1 << mx) and tab[r] is None:
            tab[r::1 << l] = [(s, l)] * (1 << (mx - l))
    return tab, mx


def _check_code(lengths, what, single_ok):
    left = 1
    for l in range(1, 16):
        left = left * 2 - sum(1 for x in lengths if x == l)
        if left < 0:
            raise DeflateError("over-subscribed %s code" % what)
    if left > 0 and not (single_ok and max(lengths, default=0) <= 1):
        raise DeflateError("incomplete %s code" % what)


def census(comp, census_into=None):
    """-> (payload, census) of the deflate stream at the start of comp; DeflateError for what RFC 1951 does not allow"""
    c = census_into if census_into is not None else new_census()
    data = bytes(comp) + b"\0" * 8
    total = 8 * len(comp)
    acc = nb = pos = 0                    # nb bits in acc; the stream's bit offset is 8 * pos - nb
    out = bytearray()
    stored_ranges = []

    def need(k):
        nonlocal acc, nb, pos
        while nb < k:
            acc |= data[pos] << nb if pos < len(data) else 0
            pos += 1
            nb += 8

    def take(k):
        nonlocal acc, nb
        need(k)
        v = acc & ((1 << k) - 1)
        acc >>= k
        nb -= k
        if 8 * pos - nb > total:
            raise DeflateError("the stream ends inside a block")
        return v

    def sym(tab, mx, what):
        nonlocal acc, nb
        need(mx)
        e = tab[acc & ((1 << mx) - 1)]
        if e is None:
            raise DeflateError("a bit pattern no %s code has" % what)
        acc >>= e[1]
        nb -= e[1]
        if 8 * pos - nb > total:
            raise DeflateError("the stream ends inside a block")
        return e

    nblocks = 0
    while True:
        at = 8 * pos - nb
        final, btype = take(1), take(2)
        if btype == 3:
            raise DeflateError("block type 3")
        c["blocks"][btype] += 1
        c["final_block"] = btype
        block_start = len(out)
        if btype == 0:
            if nblocks:
                c["stored_after_bit"].add(at & 7)
            take(nb & 7)
            n, nn = take(16), take(16)
            if n != (~nn & 0xffff):
                raise DeflateError("stored LEN / NLEN")
            b0 = (8 * pos - nb) >> 3
            if b0 + n > len(comp):
                raise DeflateError("stored bytes past the input")
            out += comp[b0:b0 + n]
            acc = nb = 0
            pos = b0 + n
            if n:
                stored_ranges.append((block_start, block_start + n))
            c.setdefault("stored_sizes", set()).add(n)
        else:
            if btype == 1:
                ll_lens, d_lens = FIXED_LL, FIXED_D
            else:
                hlit, hdist, hclen = take(5), take(5), take(4)
                c["hlit"].add(hlit)
                c["hdist"].add(hdist)
                c["hclen"].add(hclen)
                nl, nd = hlit + 257, hdist + 1
                if nl > 286 or nd > 30:
                    raise DeflateError("too many length or distance codes")
                cl_lens = [0] * 19
                for s in CLORDER[:hclen + 4]:
                    cl_lens[s] = take(3)
                _check_code(cl_lens, "code-length", False)
                tab, mx = _table(cl_lens)
                seq = []
                while len(seq) < nl + nd:
                    s, l = sym(tab, mx, "code-length")
                    c["cl_decoded"].add((s, l))
                    c["max_cl_len"] = max(c["max_cl_len"], l)
                    i = len(seq)
                    if s < 16:
                        seq.append(s)
                        continue
                    if s == 16:
                        if not seq:
                            raise DeflateError("repeat with no length before it")
                        rep, v = 3 + take(2), seq[-1]
                    elif s == 17:
                        rep, v = 3 + take(3), 0
                    else:
                        rep, v = 11 + take(7), 0
                    if i + rep > nl + nd:
                        raise DeflateError("run past the code lengths")
                    if i < nl < i + rep:
                        c["runs_across"].add(s)
                    if i + rep == nl:
                        c["runs_end_at_boundary"].add(s)
                    if i == nl:
                        c["runs_start_at_boundary"].add(s)
                    seq += [v] * rep
                ll_lens, d_lens = seq[:nl], seq[nl:]
                if ll_lens[256] == 0:
                    raise DeflateError("no end-of-block code")
                _check_code(ll_lens, "literal/length", True)
                _check_code(d_lens, "distance", True)
                c["n_dist_codes"].add(sum(1 for x in d_lens if x))
                c["ll_code_sizes"].add(sum(1 for x in ll_lens if x))
            lt, lmx = _table(ll_lens)
            dt, dmx = _table(d_lens)
            while True:
                s, l = sym(lt, lmx, "literal/length")
                if btype == 2:
                    c["ll_decoded"].add((s, l))
                    c["max_ll_len"] = max(c["max_ll_len"], l)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise DeflateError("length symbol %d" % s)
                lx = take(LEXT[s - 257])
                ds, dl = sym(dt, dmx, "distance")
                if btype == 2:
                    c["d_decoded"].add((ds, dl))
                    c["max_d_len"] = max(c["max_d_len"], dl)
                if ds > 29:
                    raise DeflateError("distance symbol %d" % ds)
                dx = take(DEXT[ds])
                length, dist = LBASE[s - 257] + lx, DBASE[ds] + dx
                if dist > len(out):
                    raise DeflateError("distance before the start of the output")
                c["lsyms"].setdefault(s, set()).add(lx)
                c["dsyms"].setdefault(ds, set()).add(dx)
                c["min_dist"] = dist if c["min_dist"] is None else min(c["min_dist"], dist)
                c["max_dist"] = dist if c["max_dist"] is None else max(c["max_dist"], dist)
                c["min_len"] = length if c["min_len"] is None else min(c["min_len"], length)
                c["max_len"] = length if c["max_len"] is None else max(c["max_len"], length)
                if dist < length:
                    c["overlaps"].add((dist, length))
                p = len(out)
                c["match_at"][p] = (dist, length, s, lx, ds, dx)
                if p - dist < block_start:
                    c["back_over_block"] += 1
                    if any(a < min(p - dist + length, p) and p - dist < b for a, b in stored_ranges):
                        c["back_into_stored"] += 1
                if dist >= length:
                    out += out[p - dist:p - dist + length]
                else:
                    for _ in range(length):
                        out.append(out[-dist])
        nblocks += 1
        if final:
            break
    c["trailing"] = len(comp) - ((8 * pos - nb + 7) >> 3)
    return bytes(out), c
