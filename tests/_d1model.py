"""A pure-Python model of how the level path treats a one-bit hybrid stream (pqg_lvd1.hpp, and the
selection rule of pqg_levels.hip k_lv_plan), so that a crafted stream can prove it has the property
its test is about before the GPU sees it.

  selected(stream, n, w)  k_lv_plan gives the page to the chunk walks (PF_D1): lv_probe_dense
                          (pqg_runs.hpp) restated, the stream length, the bit width, the
                          levels-per-byte rule and the run-only rule.
  true_chain(stream)      the headers the reference reader meets, in order.
  levels(stream, n)       how many levels the reference reads (the test compares it with the oracle).
  cause(stream, n)        why the chunk walks hand the page back, or "taken": a reading of the
                          true chain alone.
  handback(stream, n)     the three kernels' decisions replayed chunk by chunk (guesses, settle
                          rounds, restarts, entry tables, the stitch, the emit's settle): the
                          hand-back site, or None when the page is taken.

Nothing here reads the kernels' sources: the constants are restated and the CPU tests of
test_d1_model.py hold the model against the oracle's decoder.
"""
import functools
from collections import namedtuple

SEG = 16384        # D1_SEG: stream bytes per segment (one workgroup)
CH = 64            # D1_CH: stream bytes per chunk (one thread)
NCH = SEG // CH    # chunks per segment
ENT = 64           # D1_ENT: entry offsets a segment's table holds
PREK = 8           # D1_PREK: chunks of R's headers k_d1_tab keeps for the table's lanes
PROBE_SPAN = 1024  # lv_probe_dense: 64 headers within fewer bytes
PROBE_MIN = PROBE_SPAN + 64  # shortest stream that is probed at all
LPB16 = 120        # PQG_D1_LPB16: at most 120 / 16 = 7.5 levels per stream byte
RB = 131072        # D1_RB: outputs per bitmap round of k_d1_emit
DEAD = 0xFFFFFFFF    # D1_DEAD: a chain that met a header the fast parse refuses
UNKNOWN = 0xFFFFFFFE # D1_UNKNOWN: a table entry whose chain was not followed to its end

# kind: "rle" (value: the run's value byte) or "bp" (value: stream offset of the payload).
# fast: the walkers' fast parse takes the header (a varint of at most 4 bytes, header and RLE value
# or payload inside the stream). next is None for a header the reference cannot finish either.
Header = namedtuple("Header", "pos next count kind value fast")


def _byte(b, i):
    return b[i] if i < len(b) else 0


def fast_parse(b, p, slen=None, w=1):
    """lv_parse_xy at stream position p: (next, count, kind, value), or None where it refuses."""
    slen = len(b) if slen is None else slen
    vb = (w + 7) // 8
    c = [_byte(b, p + i) >> 7 for i in range(4)]
    if c[0] and c[1] and c[2] and c[3]:
        return None
    hl = 1 + c[0] + (c[0] & c[1]) + (c[0] & c[1] & c[2])
    h = 0
    for i in range(hl):
        h |= (_byte(b, p + i) & 0x7F) << (7 * i)
    g = h >> 1
    ln = hl + g * w if h & 1 else hl + vb
    if not (p < slen and ln <= slen - p):
        return None
    if h & 1:
        return p + ln, g * 8, "bp", p + hl
    return p + ln, g, "rle", int.from_bytes(bytes(_byte(b, p + hl + i) for i in range(vb)), "little")


def _vlq(b, p):
    """BitReader::get_vlq_int: (value, bytes), None when the stream ends inside it."""
    v = sh = 0
    i = p
    while i < len(b):
        x = b[i]
        i += 1
        v |= (x & 0x7F) << sh
        sh += 7
        if not x & 0x80:
            return v, i - p
    return None


def true_chain(stream):
    """The headers of the stream in the reference reader's order (RleDecoder::reload, w = 1),
    ending with the first one it cannot finish (next None)."""
    b, out, p = bytes(stream), [], 0
    while p < len(b):
        ind = _vlq(b, p)
        if ind is None:
            out.append(Header(p, None, 0, "rle", 0, False))
            break
        h, hl = ind
        fast = fast_parse(b, p) is not None
        if h & 1:
            g = h >> 1
            have = min(g, len(b) - (p + hl))  # payload bytes inside the stream
            nxt = p + hl + g if have == g else None
            out.append(Header(p, nxt, have * 8, "bp", p + hl, fast))
        elif p + hl < len(b):
            nxt = p + hl + 1
            out.append(Header(p, nxt, h >> 1, "rle", b[p + hl], fast))
        else:  # the value byte is missing
            nxt = None
            out.append(Header(p, None, 0, "rle", 0, False))
        if nxt is None:
            break
        p = nxt
    return out


def levels(stream, n):
    """Levels RleDecoder::get_batch returns for a request of n."""
    return min(n, sum(h.count for h in true_chain(stream)))


def probe_dense(stream, w=1):
    """lv_probe_dense: the first 64 headers of the stream lie within PROBE_SPAN bytes."""
    b, vb = bytes(stream), (w + 7) // 8
    q = k = 0
    while k < 64 and q + 20 < PROBE_SPAN:
        c = [_byte(b, q + i) >> 7 for i in range(4)]
        if c[0] and c[1] and c[2] and c[3]:
            break
        hl = 1 + c[0] + (c[0] & c[1]) + (c[0] & c[1] & c[2])
        h = 0
        for i in range(hl):
            h |= (_byte(b, q + i) & 0x7F) << (7 * i)
        q += hl + (h >> 1) * w if h & 1 else hl + vb
        k += 1
    return k == 64 and q < PROBE_SPAN


def run_only(stream, n, w=1):
    """lv_run_only: the first header is an RLE run of at least n levels whose value fits w bits."""
    f = fast_parse(stream, 0, w=w)
    return n > 0 and f is not None and f[2] == "rle" and f[1] >= n and (f[3] >> w) == 0


def selected(stream, n, w=1):
    """k_lv_plan flags the page PF_D1 (a def or rep stream, RLE-encoded)."""
    slen = len(stream)
    return (w == 1 and n > 0 and slen >= PROBE_MIN and probe_dense(stream, w) and n * 16 <= slen * LPB16 and
            not run_only(stream, n, w))


def segments(stream):
    return (len(stream) + SEG - 1) // SEG


def guess_entry(b, q0, cb):
    """d1_guess_entry: the exit of a walk from q0 to cb over one-byte headers, other bytes skipped."""
    slen, q = len(b), q0
    lim = min(cb, slen)
    while q < lim:
        h = b[q]
        ln = 1 + ((h >> 1) & 63) if h & 1 else 2
        one = h < 128
        q = DEAD if one and ln > slen - q else q + (ln if one else 1)
    return q


def cause(stream, n):
    """(why, stream position): the first reason the chunk walks hand the page back, in stream
    order, or ("taken", None).

      entry>=64  the chain enters a segment 64 or more bytes past its start (k_d1_stitch)
      unknown    the chain's entry into a segment does not meet R, the settled chain from chunk 0's
                 guess, within PREK chunks (k_d1_tab's table, replayed below; k_d1_stitch)
      dead       a header the fast parse refuses: a 5-byte varint, a run cut by the stream end
      value>1    an RLE run that is read holds a value above 1 (k_d1_emit)
      far        a hop over a whole chunk: next // 64 - pos // 64 >= 2 with next inside the stream,
                 from a chunk that is not its segment's last (k_d1_emit, or k_d1_tab's restart)
      short      the stream ends before n levels

    Everything counts while fewer than n levels have been met; `far` counts to the end of the
    segment in which the n-th level lies, since k_d1_emit settles that whole segment."""
    b = bytes(stream)
    slen, acc, seg, done = len(b), 0, -1, None
    for h in true_chain(b):
        j = h.pos // SEG
        if done is not None and j > done:
            break
        if done is None and j != seg:
            seg = j
            if h.pos - j * SEG >= ENT:
                return "entry>=64", h.pos
            if _tab(b, j)[4][h.pos - j * SEG][0] == UNKNOWN:
                return "unknown", h.pos
        if not h.fast:
            if done is None:
                return "dead", h.pos
            break
        if done is None and h.kind == "rle" and h.count and h.value > 1:
            return "value>1", h.pos
        if h.next // CH - h.pos // CH >= 2 and h.next < slen and (h.pos // CH) % NCH != NCH - 1:
            return "far", h.pos
        acc += h.count
        if done is None and acc >= n:
            done = j
    if done is None:
        return "short", slen
    return "taken", None


# ------------------------------------------------------------------------------ the kernels, replayed

def _walk(b, cb, q):
    """d1_walk: the chain from q through the chunk at cb: ([(header, count)], exit)."""
    slen, hs = len(b), []
    lim = min(cb + CH, slen)
    while q < lim:
        f = fast_parse(b, q)
        if f is None:
            return hs, DEAD
        hs.append((q, f[1]))
        q = f[0]
    return hs, q


def _settle(b, seg0, entry, s, W):
    """d1_settle over the segment's chunks: s[c] the entry chunk c walked from, W[c] its walk.
    Returns (last restart, far)."""
    slen = len(b)
    while True:
        outs = [w[1] for w in W]
        changed = False
        for c in range(NCH):
            cb = seg0 + c * CH
            i = entry if c == 0 else outs[c - 1]
            if i != s[c] and (i < cb + CH or (i >= slen and i != DEAD)):
                old = W[c][1]
                s[c] = i
                W[c] = _walk(b, cb, i)
                changed |= W[c][1] != old
        if not changed:
            break
    lastr = far = 0
    for c in range(NCH):
        i = entry if c == 0 else W[c - 1][1]
        if i != s[c]:
            lastr = c
            far |= i != DEAD
    return lastr, far


@functools.lru_cache(maxsize=64)
def _tab(b, j):
    """k_d1_tab for segment j: (E, s, W, lastr, table of (exit, outputs) per entry offset)."""
    slen, seg0 = len(b), j * SEG
    s, W = [], []
    for c in range(NCH):
        cb = seg0 + c * CH
        if cb >= slen:
            q, w = slen, ([], slen)
        else:
            q = 0 if cb == 0 else guess_entry(b, cb - CH, cb)
            w = _walk(b, cb, q)
        s.append(q)
        W.append(w)
    E = s[0]
    lastr, _ = _settle(b, seg0, E, s, W)
    cnt = [sum(k for _, k in w[0]) for w in W]
    suf = [0] * (NCH + 1)
    for c in range(NCH - 1, -1, -1):
        suf[c] = suf[c + 1] + cnt[c]
    pre = {}
    for c in range(PREK):
        acc = 0
        for q, k in W[c][0]:
            pre[q] = acc
            acc += k
    rexit = W[NCH - 1][1]
    tab = []
    for x in range(ENT):
        e, acc = seg0 + x, 0
        while True:
            if e >= slen:
                xo = e
                break
            k = (e - seg0) // CH
            if k >= PREK:
                xo = UNKNOWN
                break
            if e in pre:
                if k < lastr:
                    xo = DEAD
                else:
                    acc += suf[k] - pre[e]
                    xo = rexit
                break
            f = fast_parse(b, e)
            if f is None:
                xo = DEAD
                break
            acc += f[1]
            e = f[0]
        tab.append((xo, min(acc, 0xFFFFFFFF)))
    return E, s, W, lastr, tab


def handback(stream, n):
    """The hand-back site of the page (8: k_d1_stitch, 10: k_d1_emit's settle, 9: k_d1_emit's RLE
    value check), or None when the chunk walks decode it."""
    b = bytes(stream)
    slen, ns = len(b), segments(stream)
    tabs = [_tab(b, j) for j in range(ns)]
    e = jn = acc = 0
    on = []  # (segment, true entry offset)
    state = 0
    for j in range(ns):
        if state == 0 and j == jn:
            if e >= ENT:
                return 8
            xo, y = tabs[j][4][e]
            on.append((j, e))
            acc += y
            if acc >= n:
                state = 1
            elif xo >= slen:
                return 8
            else:
                jn = xo // SEG
                e = xo - jn * SEG
    if state != 1:
        return 8
    for j, x in on:  # k_d1_emit: R's walks taken over, chunk 0 from the true entry
        E, s, W, _, _ = tabs[j]
        s, W = list(s), list(W)
        entry = j * SEG + x
        if entry != E:
            s[0], W[0] = entry, _walk(b, j * SEG, entry)
        if _settle(b, j * SEG, entry, s, W)[1]:
            return 10
    acc = 0
    for h in true_chain(b):
        if acc >= n:
            break
        if h.kind == "rle" and h.count and h.value > 1:
            return 9
        acc += h.count
    return None
