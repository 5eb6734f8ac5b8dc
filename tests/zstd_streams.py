"""Hand-assembled Zstandard frames (RFC 8878) for the device page decoder (csrc/zstd_dec.h, kernels_zstd_dev.hip).

libzstd writes a narrow slice of the format; these builders write any legal frame -- RLE and repeat sequence tables, accuracy logs at
their limits, non-minimal headers, one-stream and treeless Huffman literals, directly stored weights, skippable frames, several
frames in a page -- and, for the malformed cases, one targeted illegal edit.  The plaintext is computed by applying the sequences in
Python, never by decoding the bits, so the expected output is known by construction; test_cpu_zstd_streams.py checks every case
against libzstd (through pyarrow) and against the sanitised one-lane host build of the decoder before any kernel sees it.
Plain Python and numpy, written from the RFC: nothing here touches the GPU or any zstd implementation.
"""
import bisect
import functools
import struct

import numpy as np
import xxhash

from compressed_streams import Case, _append_copy, rnd_bytes

ZSTD_MAGIC = 0xFD2FB528
SKIP_MAGIC = 0x184D2A50
BLOCK_MAX = 131072
LITW = BITW = 4096                                  # the kernel's literal and bit windows
HUFW = 256                                          # ... and each Huffman lane's

LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def _bases(first, bits):
    out = [first]
    for b in bits[:-1]:
        out.append(out[-1] + (1 << b))
    return out


LL_BASE, ML_BASE = _bases(0, LL_BITS), _bases(3, ML_BITS)
# the predefined distributions (RFC 8878 section 3.1.1.3.2.2)
LL_DEF = ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
OF_DEF = ([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1], 5)
ML_DEF = ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)
MAX_AL = {"ll": 9, "of": 8, "ml": 9}
MAX_SYM = {"ll": 36, "of": 32, "ml": 53}


def ll_code(v):
    return bisect.bisect_right(LL_BASE, v) - 1


def ml_code(v):
    return bisect.bisect_right(ML_BASE, v) - 1


# ---------------------------------------------------------------- bits
class Bits:
    """LSB-first bit writer; full 64-bit chunks leave the accumulator as they fill"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        self.acc |= v << self.n
        self.n += n
        while self.n >= 64:
            self.out += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def bytes(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) // 8, "little")


def backward(fields):
    """a bitstream that is read from its end: `fields` [(value, bits)] in the order the decoder reads them; a final 1 bit marks the end"""
    b = Bits()
    for v, n in reversed(fields):
        b.put(v, n)
    b.put(1, 1)
    return b.bytes()


# ---------------------------------------------------------------- FSE
def fse_table(norm, al):
    """the decoding table of RFC 8878 section 4.1.1: [(symbol, bits, baseline)] per state"""
    size = 1 << al
    sym, high = [0] * size, size
    for s, p in enumerate(norm):
        if p == -1:
            high -= 1
            sym[high] = s
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos >= high:
                pos = (pos + step) & (size - 1)
    assert pos == 0 and sum(abs(p) for p in norm) == size
    nxt = [1 if p == -1 else p for p in norm]
    T = []
    for i in range(size):
        d = nxt[sym[i]]
        nxt[sym[i]] += 1
        nb = al - (d.bit_length() - 1)
        T.append((sym[i], nb, (d << nb) - size))
    return T


class Fse:
    """One table (described, predefined, or the single state of RLE_Mode) and the state chooser that works backwards over it."""

    def __init__(self, norm=None, al=0, rle=None):
        self.norm, self.al = norm, al
        self.T = [(rle, 0, 0)] if rle is not None else fse_table(norm, al)
        self.by_sym = {}
        for st, (s, nb, base) in enumerate(self.T):
            self.by_sym.setdefault(s, []).append((base, nb, st))
        for v in self.by_sym.values():
            v.sort()

    def has(self, syms):
        return all(s in self.by_sym for s in syms)

    def states(self, syms, last_needs_bits=False):
        """the state that decodes each symbol: the last one free, every earlier one the state of its symbol whose range holds the next"""
        last = self.by_sym[syms[-1]]
        st = [max(last, key=lambda e: e[1])[2] if last_needs_bits else last[len(last) // 2][2]]
        for s in reversed(syms[:-1]):
            ent = self.by_sym[s]
            base, nb, state = ent[bisect.bisect_right(ent, (st[-1], 99, 0)) - 1]
            assert base <= st[-1] < base + (1 << nb)
            st.append(state)
        st.reverse()
        return st

    def step(self, a, b):
        """(value, bits) the decoder reads to go from state a to state b"""
        _, nb, base = self.T[a]
        return b - base, nb


def fse_describe(norm, al, stop_at=None):
    """the table description of section 4.1.1; stop_at: write only that many symbols (a malformed description)"""
    b = Bits()
    b.put(al - 5, 4)
    remaining, i = 1 << al, 0
    while remaining > 0 and i < (len(norm) if stop_at is None else stop_at):
        p = norm[i]
        i += 1
        x = p + 1
        bits = (remaining + 1).bit_length()
        lower, thr = (1 << (bits - 1)) - 1, (1 << bits) - 1 - (remaining + 1)
        if x < thr:
            b.put(x, bits - 1)
        elif x <= lower:
            b.put(x, bits)
        else:
            b.put(x + thr, bits)
        remaining -= abs(p)
        if p == 0:
            z = 0
            while i < len(norm) and norm[i] == 0:
                z, i = z + 1, i + 1
            while z >= 3:
                b.put(3, 2)
                z -= 3
            b.put(z, 2)
    assert stop_at is not None or remaining == 0
    return b.bytes()


def norm_for(used, al, low=()):
    """normalised counts that give every used symbol a state: those in `low` the "less than one" probability, the rest the table evenly"""
    used = sorted(set(used))
    norm = [0] * (used[-1] + 1)
    for s in used:
        norm[s] = -1 if s in low else 1
    hi = [s for s in used if s not in low]
    rest = (1 << al) - len(used)
    assert rest >= 0 and len(used) >= 2 and hi
    for k in range(rest):
        norm[hi[k % len(hi)]] += 1
    return norm


# ---------------------------------------------------------------- Huffman
def huf_lengths(n, deep=False, rng=None, limit=11):
    """code lengths of a complete prefix code with n leaves: balanced, a staircase (deep), or leaves split at random"""
    L = [1, 1]
    while len(L) < n:
        ok = [i for i, l in enumerate(L) if l < limit]
        i = max(ok, key=lambda k: L[k]) if deep else int(rng.choice(ok)) if rng is not None else min(ok, key=lambda k: L[k])
        L[i] += 1
        L.insert(i + 1, L[i])
    return L


def weights_of(symbols, lengths):
    """the weight of every byte value up to the largest symbol (0: absent)"""
    mb = max(lengths)
    w = [0] * (max(symbols) + 1)
    for s, l in zip(symbols, lengths):
        w[s] = mb + 1 - l
    return w


def huf_codes(weights):
    """{symbol: (code, bits)}: the longest codes first, symbols of one length in ascending order (section 4.2.1.3)"""
    tot = sum(1 << (w - 1) for w in weights if w)
    mb = tot.bit_length() - 1
    assert tot == 1 << mb and weights[-1] and mb <= 11
    codes, at = {}, 0
    for b in range(mb, 0, -1):
        for s, w in enumerate(weights):
            if w and mb + 1 - w == b:
                codes[s] = (at >> (mb - b), b)
                at += 1 << (mb - b)
    return codes


def huf_stream(data, codes):
    b = Bits()
    put = b.put
    for x in reversed(data):
        put(*codes[x])
    put(1, 1)
    return b.bytes()


def huf_tree_direct(weights):
    w = list(weights[:-1])
    assert 1 <= len(w) <= 128
    out = bytearray([127 + len(w)])
    w += [0] * (len(w) & 1)
    for i in range(0, len(w), 2):
        out.append((w[i] << 4) | w[i + 1])
    return bytes(out)


def huf_tree_fse(weights, al=6):
    """the weights but the last through two interleaved FSE states (section 4.2.1.2)"""
    w = list(weights[:-1])
    n = len(w)
    assert n >= 2
    hist = [w.count(v) for v in range(max(w) + 1)]
    size, present = 1 << al, [v for v, h in enumerate(hist) if h]
    assert len(present) >= 2
    norm = [max(1, h * size // n) if h else 0 for h in hist]
    big = max(present, key=lambda v: norm[v])
    norm[big] += size - sum(norm)
    assert norm[big] >= 1
    t = Fse(norm, al)
    # the read after weight n-2 has to find the stream empty: its state needs at least one bit
    a, b = w[0::2], w[1::2]
    sa = t.states(a, last_needs_bits=(n - 2) % 2 == 0)
    sb = t.states(b, last_needs_bits=(n - 2) % 2 == 1)
    assert t.T[(sa if (n - 2) % 2 == 0 else sb)[-1]][1] >= 1
    fields = [(sa[0], al), (sb[0], al)]
    for i in range(n - 2):
        ch = sa if i % 2 == 0 else sb
        fields.append(t.step(ch[i // 2], ch[i // 2 + 1]))
    body = fse_describe(norm, al) + backward(fields)
    assert len(body) < 128
    return bytes([len(body)]) + body


# ---------------------------------------------------------------- literals sections
def lit_plain(kind, data, form=None):
    """Raw_Literals_Block (kind 0) or RLE_Literals_Block (kind 1) in a 1-, 2- or 3-byte header"""
    n = len(data)
    need = 1 if n < 32 else 2 if n < 4096 else 3
    form = need if form is None else form
    assert form >= need and n < 1 << 20
    if kind == 1:
        assert n >= 1 and data == data[:1] * n
    hdr = bytes([kind | (n << 3)]) if form == 1 else (kind | 4 | (n << 4)).to_bytes(2, "little") if form == 2 else (kind | 12 | (n << 4)).to_bytes(3, "little")
    return hdr + (data if kind == 0 else data[:1])


def lit_huffman(data, codes, tree, streams=4, form=None, sizes=None):
    """Compressed_Literals_Block (tree given) or Treeless_Literals_Block (tree None); form: 10, 14 or 18 bits per size field"""
    n = len(data)
    if streams == 1:
        body = huf_stream(data, codes)
    else:
        per = (n + 3) // 4
        parts = [huf_stream(data[k * per:(k + 1) * per] if k < 3 else data[3 * per:], codes) for k in range(4)]
        assert all(len(p) < 65536 for p in parts)
        js = [len(p) for p in parts[:3]] if sizes is None else sizes
        body = struct.pack("<HHH", *js) + b"".join(parts)
    body = (tree or b"") + body
    need = 10 if max(n, len(body)) < 1 << 10 else 14 if max(n, len(body)) < 1 << 14 else 18
    form = need if form is None else {10: 14, 14: 18, 18: 18}[need] if form == "wider" else form
    assert form >= need and (streams == 4 or form == 10) and max(n, len(body)) < 1 << 18
    sf = 0 if streams == 1 else {10: 1, 14: 2, 18: 3}[form]
    v = (2 if tree is not None else 3) | (sf << 2) | (n << 4) | (len(body) << (4 + form))
    return v.to_bytes({10: 3, 14: 4, 18: 5}[form], "little") + body


# ---------------------------------------------------------------- frames
PRE, RLE, REP = ("pre",), ("rle",), ("rep",)


def FSE(norm=None, al=None, low=()):
    """Compressed_Mode: the given normalised counts, or counts made for the codes the block uses"""
    return ("fse", norm, al, tuple(low))


def rep_step(rep, ll, ofv):
    """the offset an Offset_Value stands for, and the update of the three repeat offsets (section 3.1.1.5)"""
    if ofv > 3:
        off = ofv - 3
        rep[:] = [off, rep[0], rep[1]]
        return off
    idx = ofv + (1 if ll == 0 else 0)
    if idx == 1:
        return rep[0]
    if idx == 2:
        off = rep[1]
        rep[:] = [off, rep[0], rep[2]]
    else:
        off = rep[2] if idx == 3 else rep[0] - 1
        rep[:] = [off, rep[0], rep[1]]
    return off


class ZFrame:
    """Block-by-block writer.  `blocks` holds [type, size field, payload] for targeted edits before `frame()`; `marks` the position of
    every block header in the frame; `sect` per compressed block the offsets (in its payload) of the sequences section, the modes byte,
    the table descriptions and the bitstream."""

    def __init__(self, single=False, fcs=None, checksum=False, did_bytes=0, did=0, window=0x50, reserved=0, history=b"", unchecked=False):
        self.single, self.checksum, self.did_bytes, self.did, self.window, self.reserved = single, checksum, did_bytes, did, window, reserved
        self.fcs = (1 if single else 0) if fcs is None else fcs
        assert self.fcs in (0, 1, 2, 4, 8) and (self.fcs != 1 or single) and (self.fcs != 0 or not single)
        self.blocks, self.sect, self.out = [], [], bytearray(history)      # history: a malformed frame that matches into the frame before it
        self.base, self.unchecked = len(history), unchecked
        self.rep = [1, 4, 8]
        self.prev = {"ll": None, "of": None, "ml": None}
        self.codes = None
        self.min_off, self.max_off = 1 << 40, 0

    # -- blocks
    def raw(self, data):
        assert len(data) <= BLOCK_MAX
        self.blocks.append([0, len(data), bytes(data)])
        self.sect.append(None)
        self.out += data
        return self

    def rle(self, byte, n):
        assert 1 <= n <= BLOCK_MAX
        self.blocks.append([1, n, bytes([byte])])
        self.sect.append(None)
        self.out += bytes([byte]) * n
        return self

    def pad4(self, seed=97):
        k = -len(self.out) % 4
        return self.raw(rnd_bytes(seed, k)) if k else self

    def _apply(self, literals, seqs):
        lp, out, start = 0, self.out, len(self.out)
        for ll, ofv, ml in seqs:
            assert ll >= 0 and ml >= 3 and ofv >= 1
            out += literals[lp:lp + ll]
            lp += ll
            off = rep_step(self.rep, ll, ofv)
            if self.unchecked and not 1 <= off <= len(out):
                continue                   # (a malformed case: no decoder gets this far)
            assert 1 <= off <= len(out), (off, len(out))
            self.min_off, self.max_off = min(self.min_off, off), max(self.max_off, off)
            _append_copy(out, len(out) - off, ml)
        assert lp <= len(literals)
        out += literals[lp:]
        assert len(out) - start <= BLOCK_MAX, len(out) - start

    def _table(self, which, spec, codes):
        """-> (mode, description bytes, Fse)"""
        if spec[0] == "pre":
            t = Fse(*{"ll": LL_DEF, "of": OF_DEF, "ml": ML_DEF}[which])
            return 0, b"", t
        if spec[0] == "rle":
            assert len(set(codes)) == 1
            return 1, bytes([codes[0]]), Fse(rle=codes[0])
        if spec[0] == "rep":
            assert self.prev[which] is not None and self.prev[which].has(codes)
            return 3, b"", self.prev[which]
        _, norm, al, low = spec
        if norm is None:
            used = set(codes)
            if len(used) < 2:
                used.add(0 if 0 not in used else 1)
            al = al or max(5, (len(used) - 1).bit_length())
            norm = norm_for(used, al, low)
        return 2, fse_describe(norm, al), Fse(norm, al)

    def literals_section(self, literals, lit):
        kind = lit[0]
        kw = dict(lit[1]) if len(lit) > 1 else {}
        if kind in ("raw", "rle"):
            return lit_plain(0 if kind == "raw" else 1, literals, kw.get("form"))
        if kind == "huf":
            weights = kw.pop("weights", None)
            if weights is None:
                syms = sorted(set(literals))
                weights = weights_of(syms, huf_lengths(len(syms), deep=kw.pop("deep", False), rng=kw.pop("rng", None)))
            fse = kw.pop("fse", len(weights) - 1 > 128)
            self.codes = huf_codes(weights)
            return lit_huffman(literals, self.codes, huf_tree_fse(weights) if fse else huf_tree_direct(weights), **kw)
        assert kind == "treeless" and self.codes is not None
        return lit_huffman(literals, self.codes, None, **kw)

    def block(self, literals=b"", seqs=(), lit=("raw",), ll=PRE, of=PRE, ml=PRE, count_form=None):
        """a Compressed_Block: the literals section of kind `lit`, then the sequences [(literal length, offset value, match length)]"""
        seqs = list(seqs)
        self._apply(literals, seqs)
        body = bytearray(self.literals_section(literals, lit))
        sect = {"seq": len(body)}
        n = len(seqs)
        form = (1 if n < 128 else 2 if n < 0x7F00 else 3) if count_form is None else count_form
        if form == 1:
            assert n < 128
            body.append(n)
        elif form == 2:
            assert n < 0x7F00
            body += bytes([128 + (n >> 8), n & 255])
        else:
            assert 0x7F00 <= n < 0x7F00 + 65536
            body += b"\xff" + (n - 0x7F00).to_bytes(2, "little")
        if n:
            lc, oc, mc = [ll_code(s[0]) for s in seqs], [s[1].bit_length() - 1 for s in seqs], [ml_code(s[2]) for s in seqs]
            tl, to, tm = self._table("ll", ll, lc), self._table("of", of, oc), self._table("ml", ml, mc)
            sect["modes"] = len(body)
            body.append((tl[0] << 6) | (to[0] << 4) | (tm[0] << 2))
            sect["tables"] = len(body)
            body += tl[1] + to[1] + tm[1]
            sect["bits"] = len(body)
            L, O, M = tl[2], to[2], tm[2]
            sl, so, sm = L.states(lc), O.states(oc), M.states(mc)
            fields = [(sl[0], L.al), (so[0], O.al), (sm[0], M.al)]
            for i, (llen, ofv, mlen) in enumerate(seqs):
                fields.append((ofv - (1 << oc[i]), oc[i]))
                fields.append((mlen - ML_BASE[mc[i]], ML_BITS[mc[i]]))
                fields.append((llen - LL_BASE[lc[i]], LL_BITS[lc[i]]))
                if i + 1 < n:
                    fields += [L.step(sl[i], sl[i + 1]), M.step(sm[i], sm[i + 1]), O.step(so[i], so[i + 1])]
            body += backward(fields)
            self.prev = {"ll": L, "of": O, "ml": M}
        sect["end"] = len(body)
        assert len(body) <= BLOCK_MAX, len(body)
        self.blocks.append([2, len(body), bytes(body)])
        self.sect.append(sect)
        return self

    # -- the frame
    def header(self, content_size=None):
        size = len(self.out) - self.base if content_size is None else content_size
        flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[self.fcs]
        fhd = (flag << 6) | (int(self.single) << 5) | self.reserved | (int(self.checksum) << 2) | {0: 0, 1: 1, 2: 2, 4: 3}[self.did_bytes]
        h = struct.pack("<IB", ZSTD_MAGIC, fhd)
        if not self.single:
            h += bytes([self.window])
        h += self.did.to_bytes(self.did_bytes, "little")
        if self.fcs == 2:
            assert 256 <= size < 65536 + 256
            size -= 256
        return h + (size.to_bytes(self.fcs, "little") if self.fcs else b"")

    def frame(self, content_size=None):
        assert self.blocks
        f = bytearray(self.header(content_size))
        self.marks = []
        for i, (typ, size, payload) in enumerate(self.blocks):
            self.marks.append(len(f))
            f += (int(i == len(self.blocks) - 1) | (typ << 1) | (size << 3)).to_bytes(3, "little") + payload
        if self.checksum:
            f += struct.pack("<I", xxhash.xxh64(self.plain(), seed=0).intdigest() & 0xFFFFFFFF)
        return bytes(f)

    def plain(self):
        return bytes(self.out[self.base:])


def skippable(data, nibble=0):
    return struct.pack("<II", SKIP_MAGIC + nibble, len(data)) + data


class Page:
    """frames and skippable frames back to back: what one Parquet page may carry"""

    def __init__(self):
        self.parts, self.out, self.frames = [], bytearray(), []

    def add(self, frame):
        self.parts.append(frame.frame())
        self.out += frame.plain()
        self.frames.append(frame)
        return self

    def skip(self, data, nibble=0):
        self.parts.append(skippable(data, nibble))
        return self

    def stream(self):
        return b"".join(self.parts)

    def plain(self):
        return bytes(self.out)


# ---------------------------------------------------------------- the corpus
_FACTS = {}      # name -> (smallest, largest match offset)


def facts(name):
    corpus()
    return _FACTS[name]


def _mk(name, obj, reason, expect="valid", plain=None):
    frames = [obj] if isinstance(obj, ZFrame) else obj.frames
    stream = obj.frame() if isinstance(obj, ZFrame) else obj.stream()
    plain = obj.plain() if plain is None else plain
    assert expect != "valid" or (len(plain) % 4 == 0 and len(plain) <= 410_000), (name, len(plain))
    _FACTS["zstd/" + name] = (min(f.min_off for f in frames), max(f.max_off for f in frames))
    return Case("zstd/" + name, plain, stream, "zstd", expect, reason)


def _draw(seed, n, syms):
    """n bytes over the alphabet `syms`, each symbol present when n allows"""
    a = np.asarray(list(syms), dtype=np.uint8)
    d = np.random.default_rng(seed).choice(a, n)
    d[:min(n, len(a))] = a[:min(n, len(a))]
    return d.tobytes()


def _split_blocks(f, lits, seqs, **kw):
    """the sequences in as few blocks as Block_Maximum_Size allows; lits: bytes to draw the literals from"""
    chunk, size, lp = [], 0, 0
    for s in list(seqs) + [None]:
        if s is None or size + s[0] + s[2] > BLOCK_MAX:
            n = sum(c[0] for c in chunk)
            f.block(lits[lp:lp + n], chunk, **kw)
            lp, chunk, size = lp + n, [], 0
        if s is not None:
            chunk.append(s)
            size += s[0] + s[2]
    return f


def _pattern(seed, n, const=(), max_off=37):
    """n sequences of varied codes; the tables named in `const` see one code only (RLE_Mode)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ll = 5 if "ll" in const else int(rng.choice([0, 1, 2, 7, 16, 20, 35, 70]))
        ofv = 9 if "of" in const else int(rng.choice([4, 5, 6, 10, 20, max_off + 3]))
        ml = 4 if "ml" in const else int(rng.choice([3, 4, 5, 12, 35, 40, 70, 140]))
        out.append((ll, ofv, ml))
    return out


def _lits_for(seqs, seed, extra=0):
    return rnd_bytes(seed, sum(s[0] for s in seqs) + extra)


def _fixed():
    C = []
    R = rnd_bytes

    def add(name, obj, reason):
        if isinstance(obj, ZFrame):
            obj.pad4()
        C.append(_mk(name, obj, reason))

    def small(seed, **kw):
        """a frame with a raw block and a compressed one"""
        s = [(6, 9, 5), (0, 1, 4), (3, 2, 7)]
        return ZFrame(**kw).raw(R(seed, 16)).block(_lits_for(s, seed + 1, 3), s).pad4()

    # ---- frame
    add("frame/single_segment_fcs1", ZFrame(single=True).raw(R(1, 40)), "Single_Segment_Flag: no Window_Descriptor, a 1-byte content size")
    add("frame/windowed_no_content_size", small(2), "Window_Descriptor and no content size")
    add("frame/windowed_fcs2", ZFrame(fcs=2).raw(R(3, 300)), "2-byte content size 300, stored as 44: the field holds size - 256")
    add("frame/single_fcs2_at_256", ZFrame(single=True, fcs=2).raw(R(4, 256)), "2-byte content size 256, stored as 0")
    add("frame/single_fcs2_at_65788", ZFrame(single=True, fcs=2).raw(R(5, 65788)), "2-byte content size 65788, stored as 65532: beyond 16 bits before the 256 comes off")
    add("frame/windowed_fcs4", small(6, fcs=4), "4-byte content size")
    add("frame/single_fcs4", small(7, single=True, fcs=4), "4-byte content size, single segment")
    add("frame/windowed_fcs8", small(8, fcs=8), "8-byte content size")
    add("frame/single_fcs8", small(9, single=True, fcs=8), "8-byte content size, single segment")
    add("frame/checksum", small(10, checksum=True), "Content_Checksum_Flag: four bytes after the last block (the low half of XXH64; the decoder steps over them)")
    add("frame/checksum_single_fcs2", ZFrame(single=True, fcs=2, checksum=True).raw(R(11, 400)), "checksum after a frame with a 2-byte content size")
    for nb in (1, 2, 4):
        add("frame/dictionary_id_%d_bytes_zero" % nb, small(12 + nb, did_bytes=nb), "a %d-byte Dictionary_ID field holding 0: no dictionary" % nb)
    add("frame/empty_then_data", Page().add(ZFrame(single=True).raw(b"")).add(small(17)), "an empty frame (one empty last raw block, content size 0), then a frame with data")
    add("frame/skippable_before", Page().skip(b"hello").add(small(18)), "a skippable frame (magic 0x184D2A50) in front")
    add("frame/skippable_between", Page().add(small(19)).skip(b"", 15).add(small(20)), "an empty skippable frame with magic 0x184D2A5F between two frames")
    add("frame/skippable_after", Page().add(small(21)).skip(R(22, 300), 7), "a 300-byte skippable frame at the end of the page")
    f1 = ZFrame().block(R(23, 12), [(12, 12, 6)]).pad4()
    s = [(8, 3, 5), (2, 3, 6), (1, 3, 4)]
    f2 = ZFrame(single=True).block(_lits_for(s, 24, 2), s).pad4()
    add("frame/two_frames_initial_repeat_offsets", Page().add(f1).add(f2), "the second frame's sequences use Offset_Value 3 three times: offsets 8, 4 and 1 of a fresh frame, not the 9 the first frame left")
    f2 = ZFrame().block(R(25, 20), [(20, 23, 12)]).pad4()
    f3 = ZFrame(single=True, fcs=2).raw(R(26, 300)).block(b"", [(0, 303, 40)]).pad4()
    add("frame/three_frames_offset_reaches_own_first_byte", Page().add(small(27)).add(f2).add(f3), "the second and the third frame match at an offset equal to their own output so far")
    # ---- blocks
    s = _pattern(30, 12)
    add("blocks/raw_rle_compressed_mixed", ZFrame().raw(R(31, 50)).rle(0x41, 70).block(_lits_for(s, 32, 9), s).rle(0, 5).raw(R(33, 7)).block(R(34, 10), [(4, 1, 9)]), "all three block types in one frame, twice")
    add("blocks/empty_last_raw_block", ZFrame().block(R(35, 24), [(10, 5, 6)]).raw(b""), "the last block is an empty raw block")
    add("blocks/rle_1_and_131072", ZFrame().rle(7, 1).rle(9, BLOCK_MAX).raw(R(36, 3)), "RLE blocks of 1 byte and of Block_Maximum_Size")
    s = [(3, 1, 5), (0, 1, 5), (2, 2, 5), (0, 2, 5), (1, 3, 5), (0, 3, 5)]
    f = ZFrame().raw(R(37, 40)).block(R(38, 6), [(2, 13, 4), (2, 23, 4), (2, 33, 4)]).raw(R(39, 10)).rle(3, 10).block(_lits_for(s, 40), s)
    add("blocks/repeat_offsets_across_raw_and_rle_blocks", f, "offsets 30, 20, 10 set in block 2 are the repeat offsets of block 5, a raw and an RLE block later")
    f = ZFrame().raw(R(41, 1000)).raw(R(42, BLOCK_MAX)).block(R(43, 4), [(2, BLOCK_MAX + 900 + 3, 300), (2, BLOCK_MAX + 1302 + 2 + 3, 5)])
    add("blocks/match_in_block3_from_block1", f, "a match whose source lies more than 128 KiB back, in the first block, and one that reaches byte 0")
    f = ZFrame().raw(R(44, 16))
    f.blocks.append([1, 0, b"\x00"])
    f.sect.append(None)
    add("blocks/rle_block_of_0_bytes", f.raw(R(45, 4)), "an RLE block whose Block_Size is 0: its byte is there, nothing is regenerated")
    add("blocks/compressed_block_of_0_bytes", ZFrame().raw(R(46, 16)).block(b"", []).raw(R(47, 4)), "a compressed block of two bytes: no literals, no sequences")
    # ---- raw and RLE literals
    f = ZFrame().raw(R(48, 16)).block(b"", [(0, 7, 4)])
    add("literals/rle_0_in_1_byte_header", _splice(f, 1, 0, 1, b"\x01\x5a"), "RLE literals with Regenerated_Size 0: the byte follows the header all the same")
    for kind in ("raw", "rle"):
        for size, form in ((0, 1), (30, 1), (31, 1), (5, 2), (5, 3), (32, 2), (4095, 2), (4095, 3), (4096, 3), (BLOCK_MAX, 3)):
            if kind == "rle" and size == 0:
                continue
            if kind == "raw" and size == BLOCK_MAX:
                size -= 4                  # (the block holds the 3-byte header and the sequence count as well, and may not exceed Block_Maximum_Size)
            lits = R(50 + size % 97, size) if kind == "raw" else b"\x5a" * size
            seqs = [(0, 7, 5)] if size == 0 else [] if size >= BLOCK_MAX - 4 else [(size // 2, 10, 5)]
            add("literals/%s_%d_in_%d_byte_header" % (kind, size, form), ZFrame().raw(R(51, 16)).block(lits, seqs, lit=(kind, dict(form=form))),
                "%s literals, Regenerated_Size %d in the %d-byte header%s" % (kind, size, form, " (non-minimal)" if size == 5 or (size, form) == (4095, 3) else ""))
    # ---- Huffman literals
    def huf(name, data, reason, seqs=((4, 7, 5),), **kw):
        add("huffman/" + name, ZFrame().raw(R(60, 16)).block(data, list(seqs), lit=("huf", kw)), reason)
    huf("one_stream_direct_2_weights", _draw(61, 200, range(3)), "three symbols, two weights stored directly (header byte 129)", weights=weights_of(range(3), [1, 2, 2]), streams=1)
    huf("one_stream_direct_3_weights", _draw(62, 201, range(4)), "four symbols of 2 bits, three weights stored directly", weights=weights_of(range(4), [2, 2, 2, 2]), streams=1)
    huf("direct_127_weights", _draw(63, 2002, range(128)), "128 symbols of 7 bits: 127 weights stored directly", streams=4, fse=False)
    huf("direct_128_weights", _draw(64, 2003, range(129)), "129 symbols: 128 weights stored directly, the most the header byte holds (255)", streams=4, fse=False)
    huf("direct_128_weights_sparse", _draw(65, 900, [0, 5, 64, 127, 128]), "symbols 0, 5, 64, 127, 128: weights of 0 between them", streams=1, fse=False)
    huf("fse_weights_odd_count", _draw(66, 3001, range(200)), "199 weights through the two FSE states: the last weight comes from the first state", streams=4, fse=True)
    huf("fse_weights_even_count", _draw(67, 3002, range(201)), "200 weights through the two FSE states: the last weight comes from the second state", streams=4, fse=True)
    huf("fse_weights_small_alphabet", _draw(68, 500, range(19)), "18 FSE-compressed weights of a random tree, one stream", streams=1, fse=True, rng=np.random.default_rng(68))
    huf("fse_weights_symbols_0_and_255", _draw(69, 64, [0, 255]), "two symbols with 1-bit codes, 254 weights of 0 between them", streams=1, fse=True)
    huf("two_symbols_one_bit_codes", _draw(70, 64, [0, 1]), "the smallest tree: one stored weight, 1-bit codes", streams=1)
    huf("depth_11", _draw(71, 1000, range(12)), "a staircase of 12 symbols: codes of 1 to 11 bits, the deepest tree the format allows", streams=1, deep=True)
    huf("depth_11_four_streams", _draw(72, 5000, range(40)), "40 symbols, codes up to 11 bits, four streams", streams=4, deep=True)
    huf("four_streams_10_bit_sizes", _draw(73, 600, range(16)), "Size_Format 1: four streams, 10-bit sizes", streams=4)
    huf("four_streams_14_bit_sizes", _draw(74, 5000, range(16)), "Size_Format 2: four streams, 14-bit sizes", streams=4)
    huf("four_streams_18_bit_sizes", _draw(75, 40000, range(16)), "Size_Format 3: four streams, 18-bit sizes", streams=4)
    huf("four_streams_14_bit_sizes_nonminimal", _draw(76, 600, range(16)), "sizes that fit 10 bits in the 14-bit header", streams=4, form=14)
    huf("four_streams_18_bit_sizes_nonminimal", _draw(77, 600, range(16)), "sizes that fit 10 bits in the 18-bit header", streams=4, form=18)
    huf("four_streams_18_bit_sizes_nonminimal_5000", _draw(78, 5000, range(16)), "sizes that fit 14 bits in the 18-bit header", streams=4, form=18)
    huf("four_streams_10_bit_where_one_would_do", _draw(79, 8, range(2)), "eight literals in four streams of two symbols each", streams=4)
    for n in (6, 7):
        huf("four_streams_for_%d_literals" % n, _draw(84 + n, n, range(2)), "%d literals in four streams of 2, 2, 2 and %d symbols%s" % (n, n - 6, ": the last stream is its end mark alone" if n == 6 else ""),
            seqs=((2, 7, 5),), weights=weights_of(range(2), [1, 1]), streams=4)
    for m in range(4):
        huf("four_streams_regenerated_mod4_%d" % m, _draw(80 + m, 600 + m, range(16)), "Regenerated_Size %d: the last stream holds %d symbols, the others 150 or 151" % (600 + m, 600 + m - 3 * ((600 + m + 3) // 4)), streams=4)
    flat16 = weights_of(range(16), [4] * 16)
    for nbytes in (255, 256, 257, 263, 264, 265, 271, 272, 273):
        n = 2 * (nbytes - 1)
        huf("one_stream_of_%d_bytes" % nbytes, _draw(90 + nbytes, n, range(16)), "%d 4-bit codes and the end mark: a stream of %d bytes against the %d-byte lane window" % (n, nbytes, HUFW), weights=flat16, streams=1)
        huf("four_streams_of_%d_bytes" % nbytes, _draw(91 + nbytes, 4 * n, range(16)), "four streams of %d bytes, one lane and one window each" % nbytes, weights=flat16, streams=4)
    huf("one_stream_near_1_kib", _draw(100, 1023, range(128)), "1023 literals of 7 bits: an 896-byte stream, more than three lane windows, in the one-stream form", streams=1, fse=False)
    huf("four_streams_several_windows", _draw(101, 16000, range(16)), "four streams of 2001 bytes: the lane window slides eight times", weights=flat16, streams=4)
    huf("four_streams_131072", _draw(102, BLOCK_MAX, range(16)), "Block_Maximum_Size literals: four streams of 16 KiB", seqs=(), weights=flat16, streams=4)
    f = ZFrame().block(_draw(103, 700, range(30)), [(5, 4, 5)], lit=("huf", dict(streams=4, rng=np.random.default_rng(103))))
    f.block(R(104, 50), [(9, 1, 4)]).block(_draw(105, 333, range(30)), [(5, 2, 5)], lit=("treeless", dict(streams=1))).block(_draw(106, 1500, range(30)), [(0, 1, 5)], lit=("treeless", dict(streams=4)))
    add("huffman/treeless_one_and_four_streams_after_raw_literals", f, "the tree of block 1 decodes the literals of blocks 3 (one stream) and 4 (four streams); block 2 has raw literals")
    # ---- sequence counts
    for n, form in ((0, None), (1, None), (100, 2), (127, None), (128, None), (0x7EFF, None), (0x7F00, None), (0x7F01, None)):
        seqs = [(i & 1, 4 + i % 3, 3) for i in range(n)]
        add("sequences/count_%d%s" % (n, "_in_2_bytes" if form else ""), ZFrame().raw(R(110, 8)).block(_lits_for(seqs, 111, 12), seqs, count_form=form),
            "Number_of_Sequences %d in the %d-byte form" % (n, form or (1 if n < 128 else 2 if n < 0x7F00 else 3)))
    add("sequences/count_0_in_2_bytes", ZFrame().raw(R(112, 16)).block(R(113, 12), [], count_form=2), "Number_of_Sequences 0 as the bytes 0x80 0x00: no modes byte follows")
    # ---- table modes
    rot = [(("ll",), PRE, RLE, FSE()), (("of",), FSE(), PRE, RLE), (("ml",), RLE, FSE(), PRE)]
    names = {PRE: "predefined", RLE: "rle"}
    for k in range(3):
        f = ZFrame().raw(R(120 + k, 64))
        for j in range(2):
            _, a, b, c = rot[(k + j) % 3]
            const = [w for w, m in zip(("ll", "of", "ml"), (a, b, c)) if m == RLE]
            s = _pattern(123 + k + 7 * j, 40, const)
            f.block(_lits_for(s, 124 + k, 5), s, ll=a, of=b, ml=c).block(_lits_for(s, 125 + k, 1), s, ll=REP, of=REP, ml=REP)
        a, b, c = rot[k][1:]
        add("tables/ll_%s_of_%s_ml_%s_then_repeat" % tuple(names.get(m, "described") for m in (a, b, c)), f,
            "a mode of its own for each table, Repeat_Mode for all three in the next block -- after a predefined, an RLE and a described table -- then the modes rotated, and repeated again")
    s = _pattern(130, 60)
    add("tables/accuracy_log_5", ZFrame().raw(R(131, 64)).block(_lits_for(s, 132), s, ll=FSE(al=5), of=FSE(al=5), ml=FSE(al=5)), "described tables at the smallest accuracy log")
    s = _pattern(133, 300)
    add("tables/accuracy_logs_9_8_9", ZFrame().raw(R(134, 64)).block(_lits_for(s, 135), s, ll=FSE(al=9), of=FSE(al=8), ml=FSE(al=9)).block(_lits_for(s, 136), s, ll=REP, of=REP, ml=REP),
        "described tables at the largest accuracy logs (512, 256 and 512 states), repeated in the next block")
    ll_norm = [30, 0, 0, 12] + [0] * 5 + [10] + [0] * 8 + [11, -1]
    s = [(ll, 7 + i % 5, 3 + i % 40) for i, ll in enumerate([0, 3, 9, 20, 21, 22, 23, 0, 9, 22] * 6)]
    add("tables/less_than_one_and_zero_runs", ZFrame().raw(R(137, 64)).block(_lits_for(s, 138), s, ll=FSE(ll_norm, 6), of=FSE(low=(2,)), ml=FSE(al=7, low=(0, 5, 41))),
        "literal-length counts with runs of 2, 5 and 8 zeros (one, two and three chained repeat flags) and a -1; -1 counts in the other two tables")
    # ---- every code
    f = _split_blocks(ZFrame().raw(R(140, 16)), R(141, 140_000), [(LL_BASE[c], 7, 3) for c in range(36)])
    add("codes/literal_length_0_to_35_extra_bits_zero", f, "every literal-length code at its baseline, in two blocks (code 35 alone is 65536 literals)")
    f = _split_blocks(ZFrame().raw(R(142, 16)), R(143, 140_000), [(LL_BASE[c] + (1 << LL_BITS[c]) - 1, 7, 3) for c in range(16, 35)])
    add("codes/literal_length_16_to_34_extra_bits_ones", f, "every literal-length code that has extra bits, all ones (code 35 with all ones is 131071 literals: with its match, more than a block may hold)")
    f = _split_blocks(ZFrame().raw(R(144, 16)), R(145, 60), [(1, 7, ML_BASE[c]) for c in range(53)])
    add("codes/match_length_0_to_52_extra_bits_zero", f, "every match-length code at its baseline")
    f = _split_blocks(ZFrame().raw(R(146, 16)), R(147, 60), [(1, 7, ML_BASE[c] + (1 << ML_BITS[c]) - 1) for c in range(32, 52)])
    add("codes/match_length_32_to_51_extra_bits_ones", f, "every match-length code that has extra bits, all ones (code 52 with all ones is 131074 bytes: more than a block may hold)")
    s = [(1, 1, 4), (1, 2, 4), (1, 3, 4)] + [(1, v, 4) for c in range(2, 18) for v in (1 << c, (2 << c) - 1)] + [(1, 1 << 18, 4)]
    f = ZFrame().raw(R(148, BLOCK_MAX)).raw(R(149, BLOCK_MAX)).raw(R(150, 8)).block(_lits_for(s, 151), s)
    add("codes/offset_0_to_18", f, "every offset code the page size allows, extra bits all zeros and all ones (code 18 zeros only: 262141 bytes back)")
    # ---- repeat offsets
    setup = [(2, 13, 4), (2, 23, 4), (2, 33, 4)]

    def rep(name, seqs, reason):
        s = setup + seqs
        add("repeat/" + name, ZFrame().raw(R(160, 40)).block(_lits_for(s, 161, 2), s), reason)
    rep("values_1_2_3_after_literals", [(3, 1, 5), (2, 2, 6), (1, 3, 7), (4, 3, 5), (1, 2, 5)], "Offset_Value 1, 2, 3 with literals in front: the offsets 30, 20, 10 in that order, rotated each time")
    rep("values_1_2_3_without_literals", [(0, 1, 5), (0, 2, 6), (1, 1, 3), (0, 3, 7)], "Offset_Value 1, 2 after a zero literal length mean the second and third offset; 3 means the first less one")
    rep("first_offset_minus_1", [(0, 3, 9), (0, 3, 9), (0, 3, 9)], "Offset_Value 3 without literals three times: 29, 28, 27")
    rep("same_offset_code_twice", [(1, 43, 4), (1, 43, 4), (0, 1, 6), (0, 2, 6)], "offset 40 twice in a row fills two history slots with it")
    # ---- match geometry around the 64 lanes
    for off in (1, 2, 3, 7, 63, 64, 65, 127):
        lens = sorted({max(3, n) for n in (off - 1, off, off + 1, 2 * off + 1, 3 * off + 2, 64, 200)})
        s = [(1, off + 3, ml) for ml in lens]
        add("match/offset_%d" % off, ZFrame().raw(R(170 + off, 128)).block(_lits_for(s, 171), s), "offset %d with match lengths %s: below, at and above the offset, and not a multiple of it" % (off, lens))
    s = [(1, o + 3, ml) for o in (5, 64, 100) for ml in (3, 63, 64, 65)] + [(1, 8, 65539 + 100)]
    add("match/lengths_3_63_64_65_65639", ZFrame().raw(R(180, 128)).block(_lits_for(s, 181), s), "match lengths on both sides of the 64 lanes at offsets 5, 64 and 100, and one of 65639 bytes at offset 5")
    # ---- literal window
    for kind in ("raw", "huf"):
        L = (lambda seed, n: R(seed, n)) if kind == "raw" else (lambda seed, n: _draw(seed, n, range(16)))
        spec = ("raw",) if kind == "raw" else ("huf", dict(weights=flat16, streams=4))
        s = [(0, 7, 4), (4095, 7, 4), (4096, 7, 4), (4097, 7, 4), (1, 7, 4)]
        add("litwindow/%s_runs_0_4095_4096_4097" % kind, ZFrame().raw(R(190, 16)).block(L(191, 12300), s, lit=spec), "literal runs of 0, 4095, 4096 and 4097 bytes: the last is longer than the %d-byte window" % LITW)
        s = [(4086, 7, 4), (20, 7, 4), (2, 7, 4)]
        add("litwindow/%s_run_starts_10_before_the_end" % kind, ZFrame().raw(R(192, 16)).block(L(193, 4120), s, lit=spec), "a 20-byte run that starts 10 bytes before the window's end")
        s = [(10, 7, 4)] + [(4087, 7, 4), (10, 7, 4)] * 5
        add("litwindow/%s_every_run_ends_1_past_the_window" % kind, ZFrame().raw(R(194, 16)).block(L(195, sum(x[0] for x in s) + 3), s, lit=spec),
            "runs of 4087 and 10 bytes in turn: each ends one byte past the window the run before it loaded")
        s = [(4090, 7, 4)] + [(1, 7, 3)] * 12
        add("litwindow/%s_one_byte_runs_across_the_end" % kind, ZFrame().raw(R(196, 16)).block(L(197, 4102), s, lit=spec), "1-byte runs that walk over the window's end one byte at a time")
        add("litwindow/%s_leftover_5000" % kind, ZFrame().raw(R(198, 16)).block(L(199, 5005), [(5, 7, 4)], lit=spec), "5000 literals left over after the last sequence")
    # ---- bit window
    add("bitwindow/bitstream_of_1_byte", ZFrame().raw(R(200, 16)).block(R(201, 4), [(2, 1, 3)], ll=RLE, of=RLE, ml=RLE), "three RLE tables and codes without extra bits: the bitstream is the end mark alone")
    for extra in (15, 16, 17):
        rng = np.random.default_rng(202 + extra)
        s = [(0, int(v), 3) for v in rng.integers(256, 512, BITW + extra - 1)]
        f = ZFrame().raw(R(203, 512)).block(b"", s, ll=RLE, of=RLE, ml=RLE)
        assert f.sect[-1]["end"] - f.sect[-1]["bits"] == BITW + extra
        add("bitwindow/bitstream_of_4096_plus_%d_bytes" % extra, f, "%d sequences of 8 offset bits each under RLE tables: a bitstream of exactly %d bytes against the %d + 16 bytes the window holds" % (len(s), BITW + extra, BITW))
    rng = np.random.default_rng(204)
    s = [(0, int(v), 3) for v in rng.integers(256, 512, 30000)]
    add("bitwindow/bitstream_of_30001_bytes", ZFrame().raw(R(205, 512)).block(b"", s, ll=RLE, of=RLE, ml=RLE), "30000 sequences: the window slides seven times")
    s = [(i % 3, 4 + (i * 7) % 50, 3 + i % 11) for i in range(9000)]
    add("bitwindow/9000_sequences_predefined", ZFrame().raw(R(207, 64)).block(_lits_for(s, 208), s), "9000 sequences of mixed codes in one block under the predefined tables")
    return C


def _random_block(rng, f, target, full=False):
    """one compressed block of about `target` bytes: sequences, literal kind, table modes and header widths drawn at random"""
    seqs, made, nlit, rep = [], 0, 0, list(f.rep)
    while True:
        avail = len(f.out) - f.base + made
        ll = int(rng.choice([0, 0, 1, 2, 3, 7, 15, 16, 17, 40, 300 if full else 33]))
        ml = int(rng.choice([3, 3, 4, 5, 8, 35, 36, 64, 65, 66, 131, 2000 if full else 12]))
        if avail == 0 and ll == 0:
            ll = 1
        if made + ll + ml > target - 4:
            break
        ofv = int(rng.integers(1, 4)) if rng.integers(0, 3) == 0 else 3 + int(rng.integers(1, min(avail + ll, 70 if rng.integers(0, 2) else 1 << 20) + 1))
        trial = list(rep)
        off = rep_step(trial, ll, ofv)
        if not 1 <= off <= avail + ll:
            ofv = 3 + int(rng.integers(1, avail + ll + 1))
            trial = list(rep)
            rep_step(trial, ll, ofv)
        rep = trial
        seqs.append((ll, ofv, ml))
        made, nlit = made + ll + ml, nlit + ll
    nlit += target - made
    kind = int(rng.integers(0, 5))
    if kind == 4 and f.codes is None:
        kind = 3
    if (kind >= 2 and nlit < 8) or (kind == 1 and nlit < 1):
        kind = 0
    if kind == 0:
        data = rng.integers(0, 256, nlit, dtype=np.uint8).tobytes()
        lit = ("raw", dict(form=int(rng.integers(1 if nlit < 32 else 2 if nlit < 4096 else 3, 4))))
    elif kind == 1:
        data = bytes([int(rng.integers(0, 256))]) * nlit
        lit = ("rle", dict(form=int(rng.integers(1 if nlit < 32 else 2 if nlit < 4096 else 3, 4))))
    else:
        if kind == 4:
            syms = sorted(f.codes)
        else:
            syms = sorted(int(x) for x in rng.choice(256, int(rng.integers(2, 40)), replace=False))
        a = np.asarray(syms, dtype=np.uint8)
        d = rng.choice(a, nlit)
        d[:len(a)] = a[:nlit]
        data = d.tobytes()
        streams = 1 if nlit < 1000 and rng.integers(0, 2) else 4
        kw = dict(streams=streams)
        if streams == 4 and rng.integers(0, 2):
            kw["form"] = "wider"
        if kind == 4:
            lit = ("treeless", kw)
        else:
            lit = ("huf", dict(kw, rng=rng, fse=bool(syms[-1] > 128 or (syms[-1] >= 2 and rng.integers(0, 2)))))
    modes = {}
    for which, codes in (("ll", [ll_code(s[0]) for s in seqs]), ("of", [s[1].bit_length() - 1 for s in seqs]), ("ml", [ml_code(s[2]) for s in seqs])):
        m = int(rng.integers(0, 4))
        if m == 3 and not (f.prev[which] is not None and f.prev[which].has(codes)):
            m = 2
        if m == 1 and len(set(codes)) != 1:
            m = 2
        if m == 2 and seqs:
            lo = max(5, (max(len(set(codes)), 2) - 1).bit_length())
            modes[which] = FSE(al=int(rng.integers(lo, MAX_AL[which] + 1)))
        else:
            modes[which] = (PRE, RLE, None, REP)[m] if seqs else PRE
    f.block(data, seqs, lit=lit, count_form=2 if len(seqs) < 128 and rng.integers(0, 3) == 0 else None, **modes)


def _random_cases(seed=2025, n=200, n_full=5):
    C = []
    rng = np.random.default_rng(seed)
    for i in range(n):
        single = bool(rng.integers(0, 2))
        f = ZFrame(single=single, fcs=int(rng.choice([4, 8] if single else [0, 4, 8])), checksum=bool(rng.integers(0, 2)), did_bytes=int(rng.choice([0, 0, 1, 2, 4])))
        total = int(rng.integers(13, 498)) * 4
        nb = int(rng.integers(1, 4))
        cuts = sorted(int(x) for x in rng.integers(0, total + 1, nb - 1))
        for size in np.diff([0] + cuts + [total]):
            size = int(size)
            t = int(rng.integers(0, 6))
            if t == 0 or size < 12:
                f.raw(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
            elif t == 1:
                f.rle(int(rng.integers(0, 256)), size)
            else:
                _random_block(rng, f, size)
        assert len(f.out) == total and 50 <= total <= 2000
        C.append(_mk("random_%03d" % i, f, "seeded random frame of %d blocks" % len(f.blocks)))
    for i in range(n_full):
        f = ZFrame(single=bool(i & 1), fcs=8 if i & 1 else 0, checksum=bool(i & 2))
        _random_block(rng, f, BLOCK_MAX, full=True)
        if len(f.out) < BLOCK_MAX:
            f.raw(rng.integers(0, 256, BLOCK_MAX - len(f.out), dtype=np.uint8).tobytes())
        C.append(_mk("random_full_%d" % i, f, "seeded random frame: one compressed block of 128 KiB"))
    return C


def _splice(f, bi, at, old_len, new):
    """replace old_len bytes at `at` in the payload of compressed block bi; the block header follows the new size"""
    p = f.blocks[bi][2]
    f.blocks[bi][2] = p[:at] + bytes(new) + p[at + old_len:]
    f.blocks[bi][1] = len(f.blocks[bi][2])
    return f


def _patch(stream, at, new):
    b = bytearray(stream)
    b[at:at + len(new)] = new
    return bytes(b)


_SEQS = [(5, 7, 6), (3, 12, 5), (0, 1, 4), (2, 9, 7)]


def _base(ll=PRE, of=PRE, ml=PRE, lit=("raw",), lits=None, seqs=_SEQS, **kw):
    """raw block of 16 bytes, then one compressed block (block 1); 60 bytes in all"""
    return ZFrame(**kw).raw(rnd_bytes(301, 16)).block(rnd_bytes(302, 22) if lits is None else lits, seqs, lit=lit, ll=ll, of=of, ml=ml)


def _malformed():
    """One targeted edit of a valid frame each; the reason quotes the line of csrc/zstd_dec.h that refuses it.  libzstd refuses every
    one of them as well (test_cpu_zstd_streams.py)."""
    C = []
    good = _base()
    plain, gstream = good.plain(), good.frame()
    assert len(plain) == 60

    def bad(name, stream, reason, plain=plain, expect="malformed"):
        _FACTS["zstd/bad_" + name] = (0, 0)
        C.append(Case("zstd/bad_" + name, plain, stream, "zstd", expect, reason))
    # ---- frame and block level
    bad("reserved_frame_header_bit", _base(reserved=8).frame(), "decode_frames: `if (fhd & 0x08) return false`")
    bad("truncated_in_magic", gstream[:3], "decode_frames: `if (in_len - ip < 4) return false`")
    bad("truncated_after_magic", gstream[:4], "decode_frames: `magic != 0xFD2FB528u || in_len - ip < 5`")
    bad("truncated_in_frame_header", _base(fcs=8).frame()[:9], "decode_frames: `in_len - ip < (single ? 0 : 1) + did_bytes + fcs_bytes`")
    bad("truncated_in_block_header", gstream[:good.marks[0] + 2], "decode_frames: `if (in_len - ip < 3) return false`")
    bad("truncated_after_last_block_header", gstream[:good.marks[1]] + _patch(gstream[good.marks[1]:good.marks[1] + 3], 0, bytes([gstream[good.marks[1]] & 0xFE])) + gstream[good.marks[1] + 3:],
        "decode_frames: `if (in_len - ip < 3) return false` (the last block is not marked last: a block header is expected at the end)")
    bad("truncated_in_checksum", _base(checksum=True).frame()[:-1], "decode_frames: `if (checksum) { if (in_len - ip < 4) return false; ...`")
    f = _splice(_base(lit=("raw", dict(form=3))), 1, 1, good.blocks[1][1], b"")
    bad("truncated_in_literals_header", f.frame(), "decode_block: `if (bsz < 3) return false` (a 3-byte raw literals header in a 1-byte block)")
    f = _base()
    f = _splice(f, 1, f.sect[1]["seq"], f.blocks[1][1], b"")
    bad("truncated_before_sequence_count", f.frame(), "decode_block: `if (sl < 1) return false`")
    f = _base()
    f = _splice(f, 1, f.sect[1]["seq"], f.blocks[1][1], b"\x80")
    bad("truncated_in_sequence_count", f.frame(), "decode_block: `if (sl < 2) return false` (the first byte announces the 2-byte form)")
    f = _base()
    f = _splice(f, 1, f.sect[1]["modes"], f.blocks[1][1], b"")
    bad("truncated_before_modes_byte", f.frame(), "decode_block: `if (k >= sl) return false`")
    bad("block_type_3", _patch(gstream, good.marks[1], bytes([gstream[good.marks[1]] | 6])), "decode_frames: `} else return false;` after the three block types")
    bad("block_type_3_before_a_dictionary_frame", _patch(gstream, good.marks[1], bytes([gstream[good.marks[1]] | 6])) + _base(did_bytes=1, did=5).frame(),
        "decode_frames: `} else return false;` after the three block types -- the damage comes first, so the page is malformed; the frame behind it that names a dictionary is never reached", plain=plain + plain)
    bad("raw_block_size_beyond_input", _patch(gstream, good.marks[0], (0 | (0 << 1) | (200 << 3)).to_bytes(3, "little")), "decode_frames: `bsz > in_len - ip` (a 200-byte raw block, 60 bytes left)")
    bad("compressed_block_size_beyond_input", _patch(gstream, good.marks[1], (1 | (2 << 1) | ((good.blocks[1][1] + 1) << 3)).to_bytes(3, "little")), "decode_frames: `bsz > in_len - ip` (type 2)")
    big = ZFrame().raw(rnd_bytes(303, 8))
    big.blocks.append([2, BLOCK_MAX + 4, lit_plain(0, rnd_bytes(304, BLOCK_MAX), 3) + b"\x00"])
    big.out += rnd_bytes(304, BLOCK_MAX)
    bad("compressed_block_size_beyond_128k", big.frame(), "decode_frames: `bsz > BLOCK_MAX` (a block of 131076 bytes, all of them present and otherwise in order)", plain=big.plain())
    bad("content_size_one_too_small", _base(single=True).frame(content_size=59), "decode_frames: `if (fcs >= 0 && op - frame_start != fcs) return false`")
    bad("content_size_one_too_large", _base(single=True).frame(content_size=61), "decode_frames: `if (fcs >= 0 && op - frame_start != fcs) return false` (61 announced)")
    bad("page_size_one_too_small", gstream, "decode_block: `op + rest > out_len` -- the page announces 59 bytes, the frame holds 60", plain=plain[:-1])
    bad("page_size_one_too_large", gstream, "decode_frames: `return op == out_len` -- the page announces 61 bytes", plain=plain + b"\x00")
    # ---- sequence tables
    bad("reserved_bits_in_modes_byte", _patch(gstream, good.marks[1] + 3 + good.sect[1]["modes"], b"\x01"), "decode_block: `if (modes & 3) return false`")
    bad("repeat_mode_without_a_table", _patch(gstream, good.marks[1] + 3 + good.sect[1]["modes"], b"\xfc"), "seq_table: `} else if (!*ok) return false;`")
    for which, spec in (("ll", dict(ll=FSE(al=9))), ("of", dict(of=FSE(al=8))), ("ml", dict(ml=FSE(al=9)))):
        f = _base(**spec)
        at = good.marks[1] + 3 + f.sect[1]["tables"]
        s = f.frame()
        bad("accuracy_log_%d_for_%s" % (MAX_AL[which] + 1, which), _patch(s, at, bytes([(s[at] & 0xF0) | (MAX_AL[which] + 1 - 5)])), "fse_read_table: `if (al > max_al) return -1`")
    f = _base(ll=FSE())
    f = _splice(f, 1, f.sect[1]["tables"], f.sect[1]["bits"] - f.sect[1]["tables"], fse_describe([1] * 35 + [28], 6, stop_at=35) + b"\x00")
    bad("counts_do_not_sum_to_the_table_size", f.frame(), "fse_read_table: `if (remaining != 0 || bit > nbits_total) return -1` (35 literal-length counts of 1 and a last one one short of the 29 that are left)")
    f = _base(of=FSE())
    f = _splice(f, 1, f.sect[1]["tables"], f.sect[1]["bits"] - f.sect[1]["tables"], fse_describe([1] * 33 + [31], 6, stop_at=33))
    bad("more_offset_symbols_than_the_table_allows", f.frame(), "fse_read_table: `while (remaining > 0 && symb < max_sym)` stops at 32 symbols, then `if (remaining != 0 ...) return -1`")
    for which, kw, seqs in (("ll", dict(ll=RLE), [(5, 7, 6), (5, 12, 5)]), ("of", dict(of=RLE), [(5, 9, 6), (3, 10, 5)]), ("ml", dict(ml=RLE), [(5, 7, 6), (3, 12, 6)])):
        f = _base(seqs=seqs, **kw)
        f = _splice(f, 1, f.sect[1]["tables"], 1, bytes([MAX_SYM[which]]))
        bad("rle_symbol_%d_for_%s" % (MAX_SYM[which], which), f.frame(), "seq_table: `if (sym >= max_sym) return false`", plain=f.plain())
    # ---- literals
    hl = _draw(305, 22, range(6))
    hw = weights_of(range(6), [2, 2, 3, 3, 3, 3])
    fh = _base(lit=("huf", dict(weights=hw, streams=1)), lits=hl)
    hs, hp, lit_at = fh.frame(), fh.plain(), fh.marks[1] + 3
    bad("treeless_literals_without_a_tree", _patch(hs, lit_at, bytes([hs[lit_at] | 3])), "decode_block: `} else if (!S.huf_ok) return false;`", plain=hp)
    assert hs[lit_at + 3] == 127 + 5
    bad("huffman_weight_12", _patch(hs, lit_at + 4, bytes([0xC0 | (hs[lit_at + 4] & 15)])), "huf_read_tree: `if (w[i] > 11) return -1`", plain=hp)
    bad("huffman_weights_leave_no_power_of_two", _patch(hs, lit_at + 4, b"\x11\x11\x10"), "huf_read_tree: `if (left & (left - 1)) return -1` (five weights of 1: 3 of 8 are left)", plain=hp)
    v = int.from_bytes(hs[lit_at:lit_at + 3], "little")
    bad("huffman_stream_with_bits_left_over", _patch(hs, lit_at, (v - (1 << 4)).to_bytes(3, "little")), "huf_stream: `return pos == 0` (21 symbols asked of a stream that holds 22)", plain=hp)
    bad("huffman_stream_runs_out", _patch(hs, lit_at, (v + (1 << 4)).to_bytes(3, "little")), "huf_stream: `return pos == 0` (23 symbols asked of a stream that holds 22: pos is negative)", plain=hp)
    f4 = _base(lit=("huf", dict(weights=hw, streams=4)), lits=hl)
    s4 = f4.frame()
    bad("huffman_stream_sizes_beyond_the_section", _patch(s4, lit_at + 3 + 4, b"\xff\x00"), "decode_block: `if (s4 < 1 || lastn < 0) return false` (the first of the four streams announces 255 bytes)", plain=f4.plain())
    # ---- bitstreams and sequences
    end = good.marks[1] + 3 + good.sect[1]["end"]
    bad("bitstream_last_byte_zero", _patch(gstream, end - 1, b"\x00"), "Back::init: `if (n < 1 || q[n - 1] == 0) return false`")
    cnt = good.marks[1] + 3 + good.sect[1]["seq"]
    bad("bitstream_with_bits_left_over", _patch(gstream, cnt, b"\x03"), "decode_block: `if (b.pos != 0) return false` (3 sequences asked of a bitstream that holds 4)")
    bad("bitstream_runs_dry", _patch(gstream, cnt, b"\x05"), "decode_block: `if (b.pos < 0) return false` (5 sequences asked of a bitstream that holds 4)")
    f = _base()
    f = _splice(f, 1, 0, f.sect[1]["seq"], lit_plain(0, rnd_bytes(302, 7)))
    bad("literal_lengths_beyond_the_literals", f.frame(), "decode_block: `lp + llen > regen` (7 literals, the sequences ask for 10)")
    # ---- offsets
    first = ZFrame(single=True).raw(rnd_bytes(306, 40))
    second = ZFrame(history=first.plain()).block(rnd_bytes(307, 12), [(10, 11 + 3, 4)]).pad4()
    pg = Page().add(first).add(second)
    bad("offset_reaches_into_the_previous_frame", pg.stream(), "decode_block: `(int64_t)off > op + llen - frame_start` (offset 11 after 10 bytes of the second frame)", plain=pg.plain())
    f = ZFrame(unchecked=True).raw(rnd_bytes(308, 16)).block(rnd_bytes(309, 4), [(1, 4, 3), (0, 3, 4)]).pad4()
    bad("first_repeat_offset_minus_1_is_zero", f.frame(), "decode_block: `if (off == 0 || off > 0xFFFFFFFFull) return false` (Offset_Value 3 without literals when the first offset is 1)", plain=f.plain() + bytes(4))
    # ---- unsupported
    f = _base(did_bytes=1, did=5)
    bad("dictionary_id", f.frame(), "decode_frames: `if (did_bytes && le(ip, did_bytes) != 0)` -- a dictionary is not something a Parquet page carries; the refusal sets *dictionary, the kernel raises UNPACKF_ZSTD_DICTIONARY and the scan reports the file as unsupported", expect="unsupported")
    return C


def _lenient():
    """RFC 8878 allows these, libzstd refuses them: the decoder may do either, but what it accepts must be the plaintext."""
    C = []
    w = weights_of(range(2), [1, 1])
    # four literals in four streams of one symbol each (five would be 2, 2, 2 and -1 symbols: not expressible), then a match of 5
    f = ZFrame().raw(rnd_bytes(320, 16)).block(_draw(321, 4, range(2)), [(2, 7, 5)], lit=("huf", dict(weights=w, streams=4))).pad4()
    C.append(_mk("lenient_four_streams_for_4_literals", f,
                 'section 3.1.1.3.1.1, Size_Format 01: "4 streams. Both Regenerated_Size and Compressed_Size use 10 bits (0-1023)." sets no lower bound; libzstd wants at least 6 literals for four streams',
                 expect="lenient"))
    C.append(_mk("lenient_window_of_2_to_the_41", ZFrame(window=0xF8).raw(rnd_bytes(322, 40)),
                 'section 3.1.1.1.2: "The maximum Window_Size is (1<<41) + 7*(1<<38) bytes, which is 3.75 TB" and a decoder "is allowed to reject a compressed frame that requests a memory size beyond decoder\'s authorized range"; '
                 'libzstd rejects it, this decoder keeps no window of its own and reads the 40 bytes', expect="lenient"))
    return C


@functools.lru_cache(maxsize=None)
def corpus():
    """Every case as Case(name, plaintext, stream, kind, expect, reason): the fixed table, the seeded random frames, the malformed edits,
    the dictionary frame (unsupported) and the lenient cases."""
    return tuple(_fixed() + _random_cases() + _malformed() + _lenient())


def cases(expect=None, random=None):
    return [c for c in corpus() if (expect is None or c.expect == expect) and (random is None or ("/random_" in c.name) == random)]
