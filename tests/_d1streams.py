"""The crafted one-bit level streams of test_gpu_d1.py, by name, each with what the model of
_d1model.py must say about it: whether k_lv_plan selects it for the chunk walks (PF_D1) and why,
if at all, they hand it back. test_d1_model.py proves every one of them on the CPU.

A case is built from the oracle's writer (RleEncoder through level_encode) and hand-written runs;
builders are deterministic (their own seeds).
"""
import zlib
from collections import namedtuple

import numpy as np

import _d1model as M

# selected: what _d1model.selected must say; cause: what _d1model.cause must say, a tuple of
# allowed answers, or None where the test asserts the result only.
Case = namedtuple("Case", "name stream n selected cause")

SEG, CH = M.SEG, M.CH


# ------------------------------------------------------------------------------ runs

def varint(x):
    out = bytearray()
    while True:
        b = x & 0x7F
        x >>= 7
        out.append(b | (0x80 if x else 0))
        if not x:
            return bytes(out)


def padded(x, nbytes):
    """x as a varint of exactly nbytes bytes (continuation bits over leading zero groups)."""
    return bytes(((x >> (7 * i)) & 0x7F) | (0x80 if i < nbytes - 1 else 0) for i in range(nbytes))


def run(count, value):
    return varint(count << 1) + bytes([value])


def bp(groups, payload):
    assert len(payload) == groups
    return varint((groups << 1) | 1) + bytes(payload)


def sparse(nbytes, phase=0):
    """Count-1 RLE runs of alternating value: 0.5 levels per byte."""
    assert nbytes % 2 == 0
    return b"".join(bytes([2, (phase + i) & 1]) for i in range(nbytes // 2))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def writer(oracle, rng, n, p_null):
    """The reference writer's stream of n random levels (without the v1 length prefix)."""
    lv = (rng.random(n) >= p_null).astype(np.uint64)
    return oracle.rle_encode(lv, 1)


def headers_upto(stream, limit):
    return [h.pos for h in M.true_chain(stream) if h.pos <= limit]


def prefix_to(oracle, rng, pos, p_null=0.1):
    """A writer stream cut at one of its headers and filled up with 2-byte RLE runs of 9..15
    levels to exactly `pos` bytes."""
    s = writer(oracle, rng, int(pos * 7.2) + 4000, p_null)
    assert len(s) > pos
    cut = max(q for q in headers_upto(s, pos) if (pos - q) % 2 == 0)
    s = s[:cut]
    k = 0
    while len(s) < pos:
        s += run(9 + k % 7, k & 1)
        k += 1
    assert len(s) == pos
    return s


def fill_to(s, pos):
    """2-byte RLE runs up to `pos` (an odd gap: first one run with a padded 2-byte header)."""
    assert len(s) <= pos and len(s) != pos - 1
    if (pos - len(s)) % 2:
        s += padded(11 << 1, 2) + b"\x01"
    k = 0
    while len(s) < pos:
        s += run(9 + k % 7, k & 1)
        k += 1
    return s


def total(stream):
    return sum(h.count for h in M.true_chain(stream))


# ------------------------------------------------------------------------------ taken

WRITER = [(p, n) for p in (0.1, 0.2, 0.3) for n in (20_001, 130_003, 300_007)]


def _writer(oracle, p, n):
    name = f"writer_p{p}_n{n}"
    return Case(name, writer(oracle, _rng(name), n, p), n, True, "taken")


LENGTHS = (16383, 16384, 16385, 16448, 32768)
READS = ("all", "m1", "m7", "half")


def _length_stream(oracle, slen):
    return prefix_to(oracle, _rng(f"len{slen}"), slen - 2) + run(15, 1)


def _length(oracle, slen, read, junk):
    s = _length_stream(oracle, slen)
    assert len(s) == slen
    t = total(s)
    n = {"all": t, "m1": t - 1, "m7": t - 7, "half": t // 2}[read]
    name = f"len{slen}_{read}" + ("_junk" if junk else "")
    if not junk:
        return Case(name, s, n, True, "taken")
    # the stream cut behind the run holding level n, then 40 random bytes: the reader never gets
    # there, the chunk walks may meet anything in them
    acc = 0
    for h in M.true_chain(s):
        acc += h.count
        if acc >= n:
            s = s[:h.next]
            break
    return Case(name, s + _rng(name).integers(0, 256, 40, dtype=np.uint8).tobytes(), n, None, None)


def _slen_edge(oracle, slen):
    s = prefix_to(oracle, _rng("slen_edge"), slen - 2) + run(15, 1)
    return Case(f"slen_{slen}", s, total(s), slen >= 1088, "taken" if slen >= 1088 else None)


def _lpb_edge(oracle, over):
    """More levels than 7.5 per byte in the stream (a trailing run of 2^19), read up to the rule's
    bound and one past it."""
    s = prefix_to(oracle, _rng("lpb_edge"), 3000) + padded((1 << 19) << 1, 3) + b"\x01"
    n = len(s) * M.LPB16 // 16 + over
    assert total(s) > n
    return Case(f"lpb_edge_{over}", s, n, over == 0, "taken" if over == 0 else None)


def _probe_edge(oracle, at):
    """63 bit-packed runs, then the 64th header at byte `at` (1003: the probe still parses it;
    1004: it stops one header short), a writer stream behind them."""
    rng = _rng("probe_edge")
    s = b"".join(bp(15, rng.integers(0, 256, 15, dtype=np.uint8).tobytes()) for _ in range(62))
    g = at - len(s) - 1
    s += bp(g, rng.integers(0, 256, g, dtype=np.uint8).tobytes())
    assert len(s) == at and len(M.true_chain(s)) == 63
    s += bp(7, rng.integers(0, 256, 7, dtype=np.uint8).tobytes()) + writer(oracle, rng, 30_000, 0.1)
    return Case(f"probe_edge_{at}", s, total(s), at == 1003, "taken" if at == 1003 else None)


def _tail(oracle, rng, s, n=12_000):
    return s + writer(oracle, rng, n, 0.1)


def _boundary(oracle, what, edge):
    """A header across a chunk edge (byte 64 * 40) or a segment edge (byte 16384)."""
    name = f"{what}_{edge}"
    rng = _rng(name)
    e = {"chunk": CH * 40, "segment": SEG}[edge]
    if what == "rle2":  # the value byte is the first byte behind the edge
        s = prefix_to(oracle, rng, e - 1) + run(20, 1)
    elif what == "rle3":  # a 3-byte padded header at e - 2: header bytes on both sides
        s = prefix_to(oracle, rng, e - 2) + padded(21 << 1, 3) + b"\x01"
    else:  # "bp3": the same, bit-packed, 30 groups
        s = prefix_to(oracle, rng, e - 2) + padded((30 << 1) | 1, 3) + rng.integers(0, 256, 30, dtype=np.uint8).tobytes()
    s = _tail(oracle, rng, s)
    return Case(name, s, total(s), True, "taken")


def _zero_counts(oracle):
    """Zero-count headers: 0x01 (bit-packed, no group) and 0x00 vv (an RLE run of none), single,
    and 64 x 0x01 filling exactly one chunk (every byte of it a header)."""
    rng = _rng("zero_counts")
    s = prefix_to(oracle, rng, 2000) + b"\x01" + run(9, 1) + b"\x00\x01" + run(11, 0) + b"\x00\x00" + b"\x01\x01\x01"
    s = fill_to(s, CH * 40) + b"\x01" * 64
    s = _tail(oracle, rng, s + run(13, 1))
    s = fill_to(s + b"\x00\x07", SEG + CH * 3) + b"\x01" * 64  # (a run of none: its value is never looked at)
    s = _tail(oracle, rng, s, 3000)
    return Case("zero_counts", s, total(s), True, "taken")


def _long_run(oracle, length, value, name=None, lead=1500):
    """A run of `length` levels inside a dense page, with count-1 runs around it that keep the
    page at 7.5 levels per byte or less; the run begins in the second segment at an output that
    is no multiple of 32 and spans more than one bitmap round of k_d1_emit."""
    name = name or f"long_run_{length}_{value}"
    rng = _rng(name)
    s = prefix_to(oracle, rng, lead)
    fill = (length // 7 + 2000) & ~1
    a = max(SEG + 700 - len(s), 2000) & ~1
    s += sparse(a)
    if total(s) % 32 == 0:
        s += run(1, 1)
    assert total(s) % 32 != 0 and len(s) > SEG
    s += padded(length << 1, 3) + bytes([value]) + sparse(max(fill - a, 200) & ~1, 1)
    s = _tail(oracle, rng, s, 5000)
    return Case(name, s, total(s), True, "taken")


FOREIGN = (64, 65, 100, 120, 125)


def _foreign(oracle, g):
    """A foreign writer's bit-packed run of g >= 64 groups (a 2-byte header) at a chunk's first
    byte: its hop ends in the next chunk, none is skipped."""
    name = f"foreign_bp{g}"
    rng = _rng(name)
    s = prefix_to(oracle, rng, CH * 50) + bp(g, rng.integers(0, 256, g, dtype=np.uint8).tobytes())
    s = _tail(oracle, rng, fill_to(s + run(3, 1) + run(2, 0) + run(2, 1), CH * 53 + 2))
    return Case(name, s, total(s), True, "taken")


def _foreign_seg(oracle):
    """The same in a segment's last chunk: the chain enters the next segment at offset 38."""
    rng = _rng("foreign_seg")
    s = prefix_to(oracle, rng, SEG - CH) + bp(100, rng.integers(0, 256, 100, dtype=np.uint8).tobytes())
    assert len(s) == SEG + 38
    s = _tail(oracle, rng, s)
    return Case("foreign_bp100_segment", s, total(s), True, "taken")


def _foreign_tail(oracle):
    """A run of 300 groups beginning in the last chunk of the page's last needed segment, the
    page ending inside it: no later segment is entered, and the payload's end lies past the bytes
    k_d1_emit stages (d1_bits32's loads from global memory)."""
    rng = _rng("foreign_tail")
    s = prefix_to(oracle, rng, SEG - CH + 2) + bp(300, rng.integers(0, 256, 300, dtype=np.uint8).tobytes())
    assert len(s) > SEG + 128 + 64
    return Case("foreign_bp300_tail", s, total(s) - 3, True, "taken")


# ------------------------------------------------------------------------------ handed back

def _offender(name, rng):
    """The run a hand-back case is about, and the chunk offset it must begin at (None: any)."""
    r = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    return {
        "far": (bp(64, r(64)), 62),              # 62 + 66 bytes: the next header two chunks on
        "entry64": (bp(160, r(160)), CH * 255 + 10),  # from a segment's last chunk to offset 108 of the next
        "value2": (run(20, 2), None),
        "valueFF": (run(20, 0xFF), None),
        "dead5": (b"\x90\x80\x80\x80\x00\x01", None),  # a 5-byte varint: an RLE run of 8
    }[name]


HANDBACK = {"far": "far", "entry64": "entry>=64", "value2": "value>1", "valueFF": "value>1", "dead5": "dead"}
# the hand-back site each cause means (LV_BAIL's site numbers in pqg_lvd1.hpp): 8 k_d1_stitch, 9 the
# RLE value check of k_d1_emit, 10 its settle
SITE = {"far": 10, "value>1": 9, "entry>=64": 8, "dead": 8, "unknown": 8, "short": 8}
# A hop over a chunk is met by k_d1_tab's settle first wherever the entry's chain has joined R by
# then: the chunk behind the hop is a restart, the table marks every entry that joins R before a
# restart dead, and k_d1_stitch (8) hands the page back before k_d1_emit runs. Only a hop that the
# entry's chain makes before it joins R gets to the emit's settle (10): far_emit.
SITE_OF = {"far_first": 8, "far_last": 8, "far_many": 8}


def _handback(oracle, what, where):
    """The offending run in the first segment, or in the last of three (`where`), writer levels
    around it; the page goes on behind it, into the next segment where there is one."""
    name = f"{what}_{where}"
    rng = _rng(name)
    off, at = _offender(what, rng)
    seg0 = {"first": 0, "last": 2 * SEG}[where]
    if at is None:
        pos = seg0 + CH * 100 + 17
    elif at < CH:
        pos = seg0 + CH * 100 + at
    else:
        pos = seg0 - SEG + at if where == "last" else at  # (entry64: the run ends in the segment named)
    s = prefix_to(oracle, rng, pos) + off
    s = _tail(oracle, rng, s, 90_000 if where == "first" else 12_000)  # (first: a second segment behind it)
    return Case(name, s, total(s), True, HANDBACK[what])


def _far_many(oracle):
    """200 runs of 64 groups, two short RLE runs between them, behind a writer prefix."""
    rng = _rng("far_many")
    s = prefix_to(oracle, rng, 3000)
    for k in range(200):
        s += bp(64, rng.integers(0, 256, 64, dtype=np.uint8).tobytes()) + run(3, k & 1) + run(2, ~k & 1)
    return Case("far_many", s, total(s), True, "far")


def _far_emit(oracle):
    """A hop over a chunk that only k_d1_emit's settle sees. A 3-byte padded header across the
    segment edge makes chunk 0's guess of the second segment wrong (R enters at offset 0, the true
    chain behind that run's payload); the 64-group run begins at offset 62 of the segment's first
    chunk, before the true chain has joined R, and R joins it behind the hop: the table's lane
    follows the true chain over the hop onto R, so the stitch accepts the page."""
    rng = np.random.default_rng(11)
    int(rng.integers(0, 6)), int(rng.integers(0, 2))  # (the draws of the search that found the seed)
    g = int(rng.integers(20, 50))
    s = prefix_to(oracle, rng, SEG - 2) + padded((g << 1) | 1, 3) + rng.integers(0, 256, g, dtype=np.uint8).tobytes()
    s = fill_to(s, SEG + 62) + bp(64, rng.integers(0, 256, 64, dtype=np.uint8).tobytes())
    s = _tail(oracle, rng, s, 12_000)
    return Case("far_emit", s, total(s), True, "far")


def _unknown(oracle):
    """True headers at offset 40 of every chunk (runs of 63 groups behind 1556 count-1 runs) and a
    decoy track at offset 9: payload byte 0x7F there, 0x01 elsewhere, so a walk from a chunk's
    first byte steps over one-byte zero-count headers onto the decoy and stays on it. Chunk 0's
    guess of the second segment is the decoy; the true entry's chain never meets it."""
    s = sparse(3112)
    one = bytearray(b"\x7f" + b"\x01" * 63)
    one[33] = 0x7F
    while len(s) + 64 <= 3 * SEG:
        s += bytes(one)
    return Case("unknown", s, total(s), True, "unknown")


SHORT = (1, 2, 300)
SHORT_CASES = [f"short_{c}" for c in SHORT] + [f"short_first_{c}" for c in SHORT]


def _short(oracle, cut, first):
    """A writer stream cut `cut` bytes before its end and read for all its levels: two segments,
    the cut in the second; or (`first`) one segment."""
    n = 30_001 if first else 130_003  # (one segment: still at most 7.5 levels per byte with 300 bytes cut)
    s = writer(oracle, _rng("short_first" if first else "short"), n, 0.1)
    assert M.segments(s[:-cut]) == (1 if first else 2)
    return Case(f"short_first_{cut}" if first else f"short_{cut}", s[:-cut], n, True, ("dead", "short"))


# ------------------------------------------------------------------------------ pages around a case

def v1(stream):
    return len(stream).to_bytes(4, "little") + stream


def int32_values(rng, nn):
    return rng.integers(-2 ** 31, 2 ** 31, nn, dtype=np.int64).astype(np.int32).tobytes()


def random_page(oracle, rng, n, p_null):
    """A v1 PLAIN INT32 page of n random max_def 1 levels written by the reference writer."""
    lv = (rng.random(n) >= p_null).astype(np.int16)
    return oracle.PageSpec(oracle.PAGE_DATA, oracle.level_encode(lv, 1) + int32_values(rng, int(lv.sum())), n,
                           oracle.PLAIN)


def around(oracle, spec, seed):
    """The page between two writer pages (odd level counts): its levels and values place theirs."""
    rng = np.random.default_rng(seed)
    return [random_page(oracle, rng, 20_001, 0.2), spec, random_page(oracle, rng, 9_001, 0.1)]


def rep_page(oracle, rng, n, max_def, p_rep=0.15, def_stream=None):
    """A v1 page of a max_rep 1 column: [len][rep stream][len][def stream][values]. def_stream: a
    def stream the reference cannot read to its end (n values behind it)."""
    rep = (rng.random(n) < p_rep).astype(np.int16)
    rep[0] = 0
    if def_stream is None:
        d = (rng.random(n) >= 0.2).astype(np.int16) * max_def if max_def == 1 else rng.integers(0, 3, n).astype(np.int16)
        lev, nn = oracle.level_encode(d, max_def), int((d == max_def).sum())
    else:
        lev, nn = v1(def_stream), n
    return oracle.PageSpec(oracle.PAGE_DATA, oracle.level_encode(rep, 1) + lev + int32_values(rng, nn), n, oracle.PLAIN)


def short_rep_pages(oracle, name, three):
    """The short case `name` as the def stream of a max_rep 1 page, alone or the second of three."""
    c = case(oracle, name)
    rng = np.random.default_rng(len(name))
    bad = rep_page(oracle, rng, c.n, 1, def_stream=c.stream)
    return [rep_page(oracle, rng, 20_001, 1), bad, rep_page(oracle, rng, 9_001, 1)] if three else [bad]


# ------------------------------------------------------------------------------ the catalogue

BUILDERS = {}
for _p, _n in WRITER:
    BUILDERS[f"writer_p{_p}_n{_n}"] = (lambda o, p=_p, n=_n: _writer(o, p, n))
for _l in LENGTHS:
    for _r in READS:
        for _j in (False, True):
            BUILDERS[f"len{_l}_{_r}" + ("_junk" if _j else "")] = (lambda o, l=_l, r=_r, j=_j: _length(o, l, r, j))
for _l in (1087, 1088):
    BUILDERS[f"slen_{_l}"] = (lambda o, l=_l: _slen_edge(o, l))
for _o in (0, 1):
    BUILDERS[f"lpb_edge_{_o}"] = (lambda o, v=_o: _lpb_edge(o, v))
for _a in (1003, 1004):
    BUILDERS[f"probe_edge_{_a}"] = (lambda o, a=_a: _probe_edge(o, a))
for _w in ("rle2", "rle3", "bp3"):
    for _e in ("chunk", "segment"):
        BUILDERS[f"{_w}_{_e}"] = (lambda o, w=_w, e=_e: _boundary(o, w, e))
BUILDERS["zero_counts"] = _zero_counts
BUILDERS["rle_70000_mid"] = lambda o: _long_run(o, 70_000, 1, "rle_70000_mid")
for _l in (140_000, 300_000):
    for _v in (1, 0):
        BUILDERS[f"long_run_{_l}_{_v}"] = (lambda o, l=_l, v=_v: _long_run(o, l, v))
for _g in FOREIGN:
    BUILDERS[f"foreign_bp{_g}"] = (lambda o, g=_g: _foreign(o, g))
BUILDERS["foreign_bp100_segment"] = _foreign_seg
BUILDERS["foreign_bp300_tail"] = _foreign_tail
for _w in HANDBACK:
    for _e in ("first", "last"):
        BUILDERS[f"{_w}_{_e}"] = (lambda o, w=_w, e=_e: _handback(o, w, e))
BUILDERS["far_many"] = _far_many
BUILDERS["far_emit"] = _far_emit
BUILDERS["unknown"] = _unknown
for _c in SHORT:
    BUILDERS[f"short_{_c}"] = (lambda o, c=_c: _short(o, c, False))
    BUILDERS[f"short_first_{_c}"] = (lambda o, c=_c: _short(o, c, True))

_CACHE = {}


def case(oracle, name):
    if name not in _CACHE:
        c = BUILDERS[name](oracle)
        assert c.name == name, (c.name, name)
        _CACHE[name] = c
    return _CACHE[name]
