"""Dense one-bit def / rep streams on the chunk walks (pqg_lvd1.hpp: k_d1_tab, k_d1_stitch,
k_d1_emit), and the pages they hand back to the general decoder.

k_lv_plan gives a page to the chunk walks (PF_D1, PQG_PATH_LEVEL_D1) when the density probe finds
its first 64 headers within 1 KiB, the stream has at least 1088 bytes, bit width 1 and at most 7.5
levels per byte, and is not one covering RLE run. The walks hand a page back (lv_bail: PF_D1 ->
PF_BAIL, PQG_PATH_LEVEL_HANDBACK) when the true chain meets what they do not take: a hop over a
whole 64-byte chunk, an entry into a 16 KiB segment past its first 64 bytes, a header the fast
parse refuses, an RLE value above 1, or the stream's end before n levels. A hand-back from
k_d1_emit comes after other segments of the page have stored levels and added to the page's
non-null count; k_lv_fallback then writes both again.

Every stream comes from _d1streams.py, where the CPU model (_d1model.py, test_d1_model.py) has
proved it selected or not and taken or handed back, and why. Every case decodes through the C ABI
and is compared with the oracle's read_batch: every level, every value (PLAIN INT32 unless said:
a wrong non-null count shifts every later page's values), the status and the failing page; and
every case asserts both path bits.
"""
import numpy as np
import pytest

import _d1streams as S
from test_gpu_level_runs import _equal, _page, _random_page, _ref_bad_page

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import pqgpu
    c = pqgpu.Context(0)
    yield c
    c.close()


def _bits(paths):
    import pqgpu
    return bool(paths & pqgpu.PATH_LEVEL_D1), bool(paths & pqgpu.PATH_LEVEL_HANDBACK)


def _check(oracle, ctx, specs, d1, handback, ptype=None, max_def=1, max_rep=0, misalign=0, what=""):
    """Decode the chunk, compare with the oracle, assert the two path bits (None: not asserted)."""
    import pqgpu
    ptype = oracle.INT32 if ptype is None else ptype
    kw = dict(max_def=max_def, max_rep=max_rep)
    ref = oracle.read_column(ptype, specs, **kw)
    got = pqgpu.decode_column(ctx, ptype, specs, misalign=misalign, **kw)
    paths = ctx.last_paths()
    _equal(oracle, ptype, got, ref, max_def, max_rep, what)
    if ref["status"]:
        assert got["page"] == _ref_bad_page(oracle, ptype, specs, **kw), (what, got["page"])
    g1, ghb = _bits(paths)
    assert d1 is None or g1 == d1, (what, "LEVEL_D1", paths)
    assert handback is None or ghb == handback, (what, "LEVEL_HANDBACK", paths)
    return got, ref


def _case_page(oracle, name, **kw):
    c = S.case(oracle, name)
    return _page(oracle, np.random.default_rng(len(name)), c.stream, c.n, **kw)


_around, _rep_page = S.around, S.rep_page


# ------------------------------------------------------------------------------ taken: writer streams

@pytest.mark.parametrize("p_null,n", S.WRITER)
def test_writer_pages(oracle, ctx, p_null, n):
    """The reference writer's streams at p_null 0.1 / 0.2 / 0.3, one, two and three segments."""
    got, ref = _check(oracle, ctx, [_case_page(oracle, f"writer_p{p_null}_n{n}")], True, False)
    assert ref["status"] == 0 and len(ref["def"]) == n


def _three(oracle, **kw):
    return [_case_page(oracle, f"writer_p{p}_n{n}", **kw) for p, n in ((0.1, 20_001), (0.2, 130_003), (0.3, 20_001))]


def test_three_pages_at_odd_output_offsets(oracle, ctx):
    """Three pages in one chunk: the second and third pages' levels begin at outputs 20 001 and
    150 004, no multiples of 8 or 32 (the bitmap's word and the 16-byte stores' alignment)."""
    _check(oracle, ctx, _three(oracle), True, False)


@pytest.mark.parametrize("misalign", [1, 7, 15])
def test_misaligned_payloads(oracle, ctx, misalign):
    _check(oracle, ctx, _three(oracle), True, False, misalign=misalign, what=misalign)


def test_v2_pages(oracle, ctx):
    """DataPageV2: the def stream is def_len bytes without a length prefix."""
    _check(oracle, ctx, _three(oracle, v2=True), True, False)


def test_int64_values(oracle, ctx):
    _check(oracle, ctx, _three(oracle, ptype=oracle.INT64), True, False, ptype=oracle.INT64)


# ------------------------------------------------------------------------------ taken: the rule's edges

@pytest.mark.parametrize("name", ["slen_1087", "slen_1088", "lpb_edge_0", "lpb_edge_1", "probe_edge_1003",
                                  "probe_edge_1004"])
def test_selection_edges(oracle, ctx, name):
    """Both sides of each term of the rule: 1087 / 1088 stream bytes; n = slen * 120 // 16 levels
    and one more, of one stream; the 64th header at byte 1003 (the probe parses it) and at 1004."""
    c = S.case(oracle, name)
    _check(oracle, ctx, [_case_page(oracle, name)], c.selected, False, what=name)
    _check(oracle, ctx, _around(oracle, _case_page(oracle, name), 1), True, False, what=name)  # (the writer pages)


@pytest.mark.parametrize("read", S.READS)
@pytest.mark.parametrize("slen", S.LENGTHS)
def test_stream_length_edges(oracle, ctx, slen, read):
    """Streams of exactly 16 383 .. 32 768 bytes (one segment to the byte, one byte and one chunk
    more, two segments), read to their last level, 1 and 7 levels short of it (the last run read in
    part) and half (trailing segments off the chain, trailing bytes never read). Then cut behind
    the last run read with 40 random bytes after it: the reader never sees them, the chunk walks
    may; a hand-back is allowed there, the result is not."""
    name = f"len{slen}_{read}"
    _check(oracle, ctx, [_case_page(oracle, name)], True, False, what=name)
    _check(oracle, ctx, _around(oracle, _case_page(oracle, name + "_junk"), 2), True, None, what=name + "_junk")


@pytest.mark.parametrize("name", ["rle2_chunk", "rle2_segment", "rle3_chunk", "rle3_segment", "bp3_chunk", "bp3_segment",
                                  "zero_counts", "rle_70000_mid"])
def test_headers_on_boundaries(oracle, ctx, name):
    """A 2-byte RLE run whose value byte is the next chunk's / segment's first byte; 3-byte padded
    headers (RLE, bit-packed) across those edges; zero-count headers, 64 of them filling a chunk;
    an RLE run with a 3-byte count of 70 000 in mid-stream."""
    _check(oracle, ctx, [_case_page(oracle, name)], True, False, what=name)
    _check(oracle, ctx, _around(oracle, _case_page(oracle, name), 3), True, False, what=name)


@pytest.mark.parametrize("value", [1, 0])
@pytest.mark.parametrize("length", [140_000, 300_000])
def test_long_rle_runs_inside_a_page(oracle, ctx, length, value):
    """A run of more levels than one bitmap round of k_d1_emit holds (131 072), beginning at an
    output that is no multiple of 32, of ones and of zeros, count-1 runs keeping the page dense."""
    name = f"long_run_{length}_{value}"
    got, ref = _check(oracle, ctx, _around(oracle, _case_page(oracle, name), 4), True, False, what=name)
    assert ref["status"] == 0


@pytest.mark.parametrize("name", [f"foreign_bp{g}" for g in S.FOREIGN] + ["foreign_bp100_segment", "foreign_bp300_tail"])
def test_foreign_long_bit_packed_runs_are_taken(oracle, ctx, name):
    """Bit-packed runs of 64 and more groups (2-byte headers: legal, not the reference writer's)
    that skip no chunk: at a chunk's first byte; in a segment's last chunk, entering the next
    segment at offset 38; and 300 groups in the last chunk of the last needed segment, the payload
    read from global memory past the staged bytes."""
    _check(oracle, ctx, [_case_page(oracle, name)], True, False, what=name)
    _check(oracle, ctx, _around(oracle, _case_page(oracle, name), 5), True, False, what=name)


@pytest.mark.parametrize("max_def", [2, 1])
def test_rep_levels(oracle, ctx, max_def):
    """max_rep 1: a dense one-bit rep stream beside def levels of bit width 2 (the rep stream alone
    takes the chunk walks), and beside a dense one-bit def stream (both do)."""
    rng = np.random.default_rng(60 + max_def)
    specs = [_rep_page(oracle, rng, n, max_def) for n in (20_001, 130_003, 9_001)]
    got, ref = _check(oracle, ctx, specs, True, False, max_def=max_def, max_rep=1)
    assert ref["status"] == 0 and ref["rep"].any()


# ------------------------------------------------------------------------------ handed back

@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("what", sorted(S.HANDBACK))
def test_handed_back(oracle, ctx, what, where):
    """One offending run in a writer page's first segment, or in the last of three (the earlier
    segments have emitted their levels and counted their ones by then): a 64-group run from chunk
    offset 62 (far), a 160-group run from a segment's last chunk (entry>=64), RLE runs of value 2
    and 0xFF (the reference returns the value as the level), a 5-byte varint header (dead). As a
    chunk of its own and between two writer pages."""
    name = f"{what}_{where}"
    got, ref = _check(oracle, ctx, [_case_page(oracle, name)], True, True, what=name)
    assert ref["status"] == 0
    _check(oracle, ctx, _around(oracle, _case_page(oracle, name), 6), True, True, what=name)


@pytest.mark.parametrize("name", ["far_many", "far_emit", "unknown"])
def test_handed_back_streams(oracle, ctx, name):
    """far_many: 200 runs of 64 groups behind a writer prefix. far_emit: a hop over a chunk that the
    true chain makes before it joins R, so that the stitch accepts the page and k_d1_emit's settle
    hands it back (the other far cases are met by k_d1_tab's restart and the stitch). unknown:
    three segments of 63-group runs at chunk offset 40 with a decoy header track at offset 9, which
    chunk 0's guess follows."""
    got, ref = _check(oracle, ctx, [_case_page(oracle, name)], True, True, what=name)
    assert ref["status"] == 0
    _check(oracle, ctx, _around(oracle, _case_page(oracle, name), 7), True, True, what=name)


@pytest.mark.parametrize("rep", [False, True])
@pytest.mark.parametrize("name", S.SHORT_CASES)
def test_stream_ends_before_its_levels(oracle, ctx, name, rep):
    """A def stream cut 1, 2 and 300 bytes before its end: two segments with the cut in the second,
    and one segment. As a chunk of its own (the failing page is page 0, nothing before it) and as
    the second of three pages.

    Without rep levels: the oracle's status on that page (HANG: the level decoder spins on a
    bit-packed run whose payload is cut, or returns a short batch after which read_batch makes no
    progress). With rep levels (max_rep 1, a whole dense rep stream beside the cut def stream) the
    reference hangs the same way or panics on differing def / rep counts, and the decoder reports
    EOF on that page: the deviation DESIGN section 4 lists for level streams that end early in
    columns with rep levels. The test holds it to exactly that: the oracle fails with HANG or
    PANIC on the page, the GPU with EOF on the same page."""
    import pqgpu
    for three in (False, True):
        bad = int(three)
        if not rep:
            spec = _case_page(oracle, name)
            got, ref = _check(oracle, ctx, _around(oracle, spec, 8) if three else [spec], True, True, what=(name, three))
            assert ref["status"] == pqgpu.HANG and got["page"] == bad, (name, three)
            continue
        specs = S.short_rep_pages(oracle, name, three)
        kw = dict(max_def=1, max_rep=1)
        ref = oracle.read_column(oracle.INT32, specs, **kw)
        got = pqgpu.decode_column(ctx, oracle.INT32, specs, **kw)
        assert _bits(ctx.last_paths()) == (True, True), (name, three)
        assert ref["status"] in (pqgpu.HANG, pqgpu.PANIC), (name, three, ref["status"])
        assert _ref_bad_page(oracle, oracle.INT32, specs, **kw) == bad, (name, three)
        assert got["status"] == pqgpu.EOF and got["page"] == bad, (name, three, got["status"], got["message"])


# ------------------------------------------------------------------------------ state that outlives a decode

def test_stale_tables_between_decodes(oracle, ctx):
    """One context: a three-segment page, a one-segment page, a handed-back page, the first again.
    The segment records (tables, stitch results, R's walks) outlive a decode."""
    three, one = [_case_page(oracle, "writer_p0.1_n300007")], [_case_page(oracle, "writer_p0.2_n20001")]
    back = [_case_page(oracle, "value2_last")]
    for specs, hb in ((three, False), (one, False), (back, True), (three, False), (back, True), (one, False)):
        _check(oracle, ctx, specs, True, hb)


class _Job:
    """One pqg_decode_chunks call of fixed-width PLAIN chunks (ptype, specs, max_def) in flight,
    the 8 guard levels behind each chunk's last page pre-filled with a sentinel."""

    def __init__(self, ctx, chunks):
        import torch

        import pqgpu
        self.chunks, self.keep, arrays, parts, off = chunks, [], [], [], 0
        for ptype, specs, max_def in chunks:
            arr = (pqgpu.Page * len(specs))()
            for i, s in enumerate(specs):
                pad = (-off) % 64
                parts.append(b"\0" * pad)
                off += pad
                arr[i] = pqgpu.Page(off, len(s.buf), s.num_values, s.page_type, s.encoding, s.def_encoding,
                                    s.rep_encoding, s.def_len, s.rep_len)
                parts.append(s.buf)
                off += len(s.buf)
            arrays.append(arr)
        blob = b"".join(parts) + b"\0" * 64
        self.d_blob = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        cols, outs = [], []
        for ptype, specs, max_def in chunks:
            nlev = sum(s.num_values for s in specs)
            cap = nlev * pqgpu.VALUE_SIZE[ptype]
            d_def = torch.full((nlev + 8,), SENTINEL, dtype=torch.int16, device="cuda")
            d_val = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
            cols.append(pqgpu.Column(ptype, -1, max_def, 0))
            outs.append(pqgpu.Output(d_def.data_ptr(), None, d_val.data_ptr(), cap, None, 0, 0, 0, 0))
            self.keep.append((d_def, d_val, nlev))
        self.oa = ctx.decode_chunks_async(cols, self.d_blob.data_ptr(), len(blob), arrays, outs,
                                          torch.cuda.current_stream().cuda_stream)

    def check(self, oracle, what=""):
        """After the sync: every chunk against the oracle, and no level written past its last page."""
        import pqgpu
        for k, (ptype, specs, max_def) in enumerate(self.chunks):
            ref = oracle.read_column(ptype, specs, max_def=max_def)
            assert ref["status"] == 0, ref["message"]
            d_def, d_val, nlev = self.keep[k]
            o = self.oa[k]
            assert o.num_levels == len(ref["def"]) == nlev and o.num_values == len(ref["values"]), (what, k)
            np.testing.assert_array_equal(d_def[:nlev].cpu().numpy(), ref["def"], err_msg=f"{what} chunk {k}")
            assert (d_def[nlev:].cpu().numpy() == SENTINEL).all(), (what, k, "levels written past the last page")
            got = d_val[:o.num_values * pqgpu.VALUE_SIZE[ptype]].cpu().numpy().tobytes()
            assert got == np.asarray(ref["values"]).tobytes(), (what, k)


def test_alternating_batches_use_both_slots(oracle, ctx):
    """Two batches enqueued alternately without a sync between them (the context's two slots):
    taken pages in one; a handed-back page with a window-path page (p_null 0.03) behind it, and a
    taken INT64 chunk, in the other. The bits are the last decode's."""
    rng = np.random.default_rng(70)
    a = [(oracle.INT32, _three(oracle), 1), (oracle.INT32, [_case_page(oracle, "len16384_m7")], 1)]
    b = [(oracle.INT32, [_case_page(oracle, "far_last"), S.random_page(oracle, rng, 50_001, 0.03)], 1),
         (oracle.INT64, [_case_page(oracle, "foreign_bp300_tail", ptype=oracle.INT64)], 1)]
    for rnd in range(2):
        ja = _Job(ctx, a)
        jb = _Job(ctx, b)
        st = ctx.sync_detail()
        assert st[0] == 0, (rnd, st, ctx.error_message())
        assert _bits(ctx.last_paths()) == (True, True)  # (the last decode's: b)
        ja.check(oracle, ("a", rnd))
        jb.check(oracle, ("b", rnd))
        jb2 = _Job(ctx, b)
        ja2 = _Job(ctx, a)
        st = ctx.sync_detail()
        assert st[0] == 0, (rnd, st, ctx.error_message())
        assert _bits(ctx.last_paths()) == (True, False)  # (a)
        jb2.check(oracle, ("b2", rnd))
        ja2.check(oracle, ("a2", rnd))


def test_taken_handed_back_and_wide_chunks_in_one_batch(oracle, ctx):
    """One pqg_decode_chunks: a taken chunk, a handed-back chunk (the page in the middle) and a
    max_def 3 chunk: one pass of every kernel over the three."""
    rng = np.random.default_rng(71)
    wide = [_random_page(oracle, rng, 30_001, 0.4, 3, ptype=oracle.INT64),
            _random_page(oracle, rng, 999, 0.1, 3, ptype=oracle.INT64)]
    job = _Job(ctx, [(oracle.INT32, _three(oracle), 1),
                     (oracle.INT32, _around(oracle, _case_page(oracle, "entry64_last"), 9), 1),
                     (oracle.INT64, wide, 3)])
    st = ctx.sync_detail()
    assert st[0] == 0, (st, ctx.error_message())
    assert _bits(ctx.last_paths()) == (True, True)
    job.check(oracle)
