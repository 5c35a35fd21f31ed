"""Hybrid streams that are one RLE run (k_lv_plan's run-only rule, pqg_levels.hip lv_run_only).

A def / rep / RLE-boolean / dictionary-index stream whose first header is an RLE run holding every
output the reader asks for ("nullable column, no nulls in this page", an all-null page, a flat
list's rep levels) is settled by the level path's plan kernel: the page becomes a walked page
without segment starts, walks, page scan or run compaction, and the decode reports
PQG_PATH_LEVEL_RUNS. The reader stops at n outputs (RleDecoder::get_batch, rle.rs:398-434), so
whatever follows the run is never read. Every other first header (count 0, a shorter run, a value
wider than the bit width, a cut header) stays on the paths that reproduce the reference's errors.

Every case decodes through the C ABI and is compared with the oracle's read_batch: every level,
every value, the status and the failing page (the oracle's failing page: the first page prefix
of the chunk it fails on).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import pqgpu
    c = pqgpu.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------ hand-written streams

def _varint(x):
    out = bytearray()
    while True:
        b = x & 0x7F
        x >>= 7
        out.append(b | (0x80 if x else 0))
        if not x:
            return bytes(out)


def _run(count, value, w):
    """An RLE run: varint(count << 1), then the value in ceil(w / 8) bytes (rle.rs:167-178)."""
    return _varint(count << 1) + int(value).to_bytes((w + 7) // 8, "little")


def _bp(groups, payload):
    """A bit-packed run header of `groups` groups of 8 values, then its payload."""
    return _varint((groups << 1) | 1) + payload


def _v1(stream):
    return len(stream).to_bytes(4, "little") + stream


def _width(max_level):
    return max(1, int(max_level).bit_length())


def _levels_of(oracle, stream, w, n):
    """The levels the reference reads from `stream`, or None when it fails."""
    st, lv = oracle.rle_decode(stream, w, n, type_size=2)
    return lv if st == 0 and len(lv) == n else None


def _values(oracle, rng, ptype, nn):
    if ptype == oracle.INT32:
        return rng.integers(-2 ** 31, 2 ** 31, nn, dtype=np.int64).astype(np.int32).tobytes()
    if ptype == oracle.INT64:
        return rng.integers(-2 ** 62, 2 ** 62, nn, dtype=np.int64).tobytes()
    if ptype == oracle.INT96:
        return rng.integers(0, 256, nn * 12, dtype=np.uint8).tobytes()
    assert ptype == oracle.BYTE_ARRAY
    a = np.frombuffer(b"abcdefghijklmnop", np.uint8)
    return oracle.plain_encode_ba([bytes(a[rng.integers(0, 16, l)]) for l in rng.integers(0, 20, nn)])


def _page(oracle, rng, stream, n, max_def=1, ptype=None, v2=False, nvals=None):
    """A PLAIN data page behind the def stream `stream` (v1: [i32 len][stream]; v2: def_len), with
    the values of its levels == max_def (n values when the reference cannot read the stream)."""
    ptype = oracle.INT32 if ptype is None else ptype
    if nvals is None:
        lv = _levels_of(oracle, stream, _width(max_def), n)
        nvals = n if lv is None else int((lv == max_def).sum())
    body = _values(oracle, rng, ptype, nvals)
    if v2:
        return oracle.PageSpec(oracle.PAGE_DATA_V2, stream + body, n, oracle.PLAIN, def_len=len(stream))
    return oracle.PageSpec(oracle.PAGE_DATA, _v1(stream) + body, n, oracle.PLAIN)


def _random_page(oracle, rng, n, p_null, max_def=1, ptype=None):
    ptype = oracle.INT32 if ptype is None else ptype
    lv = (rng.random(n) >= p_null).astype(np.int16) * max_def
    body = _values(oracle, rng, ptype, int((lv == max_def).sum()))
    return oracle.PageSpec(oracle.PAGE_DATA, oracle.level_encode(lv, max_def) + body, n, oracle.PLAIN)


# ------------------------------------------------------------------------------ comparison

def _ref_bad_page(oracle, ptype, specs, **kw):
    """The page the reference fails on: the first prefix of the chunk's pages it cannot read."""
    for k in range(len(specs)):
        if oracle.read_column(ptype, specs[:k + 1], **kw)["status"]:
            return k
    return -1


def _equal(oracle, ptype, got, ref, max_def, max_rep, what=""):
    assert got["status"] == ref["status"], (what, got["status"], got["message"], ref["status"], ref["message"])
    if ref["status"]:
        return
    if max_def > 0:
        np.testing.assert_array_equal(got["def"], ref["def"], err_msg=str(what))
    if max_rep > 0:
        np.testing.assert_array_equal(got["rep"], ref["rep"], err_msg=str(what))
    assert got["num_values"] == len(ref["values"]), what
    if ptype == oracle.BYTE_ARRAY:
        assert got["bytes"] == ref["bytes"], what
        np.testing.assert_array_equal(got["offsets"], ref["offsets"], err_msg=str(what))
    else:
        assert np.asarray(got["values"]).tobytes() == np.asarray(ref["values"]).tobytes(), what


def _check(oracle, ctx, specs, runs, ptype=None, max_def=1, max_rep=0, misalign=0, what=""):
    """Decode the chunk, compare with the oracle, and assert whether the run-only path took a page."""
    import pqgpu
    ptype = oracle.INT32 if ptype is None else ptype
    kw = dict(max_def=max_def, max_rep=max_rep)
    ref = oracle.read_column(ptype, specs, **kw)
    got = pqgpu.decode_column(ctx, ptype, specs, misalign=misalign, **kw)
    paths = ctx.last_paths()
    _equal(oracle, ptype, got, ref, max_def, max_rep, what)
    if ref["status"]:
        assert got["page"] == _ref_bad_page(oracle, ptype, specs, **kw), (what, got["page"])
    assert bool(paths & pqgpu.PATH_LEVEL_RUNS) == runs, (what, paths)
    return got, ref


# ------------------------------------------------------------------------------ the path is taken

@pytest.mark.parametrize("value", [1, 0])
@pytest.mark.parametrize("n", [1, 7, 8, 4095, 4096, 4097, 70_000])
def test_one_run_sizes(oracle, ctx, n, value):
    """max_def 1, one run of exactly n levels: all present (n values) or all null (none)."""
    rng = np.random.default_rng(n + value)
    got, ref = _check(oracle, ctx, [_page(oracle, rng, _run(n, value, 1), n)], True)
    assert ref["status"] == 0 and len(ref["def"]) == n and got["num_values"] == n * value


@pytest.mark.parametrize("tail", [0, 1, 37, 3000])
def test_run_longer_than_page_and_trailing_bytes(oracle, ctx, tail):
    """A run of 2^20 levels read by a page of 4097 (a three-byte varint), and bytes after the run:
    the reader never reaches them (37: inside the first window; 3000: three windows, and long enough
    for the density probe to look at them)."""
    rng = np.random.default_rng(tail)
    junk = rng.integers(0, 256, tail, dtype=np.uint8).tobytes()
    _check(oracle, ctx, [_page(oracle, rng, _run(1 << 20, 1, 1) + junk, 4097, nvals=4097)], True, what=tail)
    _check(oracle, ctx, [_page(oracle, rng, _run(4097, 0, 1) + junk, 4097, nvals=0)], True, what=tail)


@pytest.mark.parametrize("max_def,value", [(2, 0), (2, 2), (2, 1), (3, 0), (3, 3), (3, 2), (255, 255), (255, 0),
                                           (255, 17), (300, 300), (300, 256)])
def test_wider_levels(oracle, ctx, max_def, value):
    """Bit widths 2 (max_def 2, 3), 8 (255) and 9 (300: a two-byte run value): the run's value is 0,
    max_def (every level a value) or another level below it."""
    rng = np.random.default_rng(max_def * 1000 + value)
    n = 5001
    got, _ = _check(oracle, ctx, [_page(oracle, rng, _run(n, value, _width(max_def)), n, max_def=max_def)], True,
                    max_def=max_def)
    assert got["num_values"] == (n if value == max_def else 0)


def test_v2_pages(oracle, ctx):
    """DataPageV2: the def stream is def_len bytes without a length prefix."""
    rng = np.random.default_rng(2)
    specs = [_page(oracle, rng, _run(n, v, 1), n, v2=True) for n, v in ((4097, 1), (300, 0), (9, 1))]
    _check(oracle, ctx, specs, True)


def test_rep_stream_of_one_run(oracle, ctx):
    """A max_rep 1 column whose rep levels are one run of 0 (a list column of one-element lists)
    beside random def levels of bit width 2: the rep stream takes the path, the def stream not."""
    rng = np.random.default_rng(3)
    specs = []
    for n in (6000, 4097):
        d = rng.integers(0, 3, n).astype(np.int16)
        body = _values(oracle, rng, oracle.INT32, int((d == 2).sum()))
        specs.append(oracle.PageSpec(oracle.PAGE_DATA, _v1(_run(n, 0, 1)) + oracle.level_encode(d, 2) + body, n,
                                     oracle.PLAIN))
    got, ref = _check(oracle, ctx, specs, True, max_def=2, max_rep=1)
    assert not ref["rep"].any() and len(ref["rep"]) == 10097


@pytest.mark.parametrize("tname", ["INT32", "INT64", "INT96", "BYTE_ARRAY"])
def test_value_types(oracle, ctx, tname):
    """All-present, all-null and all-present pages of each PLAIN value type (INT96: 12-byte values)."""
    rng = np.random.default_rng(len(tname))
    ptype = getattr(oracle, tname)
    specs = [_page(oracle, rng, _run(n, v, 1), n, ptype=ptype) for n, v in ((4097, 1), (1000, 0), (4095, 1))]
    _check(oracle, ctx, specs, True, ptype=ptype)


@pytest.mark.parametrize("max_def", [0, 1])
def test_dictionary_indices_of_one_run(oracle, ctx, max_def):
    """An RLE_DICTIONARY page whose index stream ([bit width][hybrid], decoding.rs:292-300) is one
    run: every value the same dictionary entry. max_def 0: the index stream alone decides the path
    bit; max_def 1: behind random def levels, the run shorter than the page's levels."""
    rng = np.random.default_rng(4 + max_def)
    dvals = rng.integers(-10 ** 12, 10 ** 12, 5)
    d = oracle.PageSpec(oracle.PAGE_DICTIONARY, oracle.plain_encode(oracle.INT64, dvals), 5, oracle.PLAIN_DICTIONARY)
    specs = [d]
    for n, entry in ((5000, 4), (4097, 0)):
        if max_def:
            lv = (rng.random(n) >= 0.3).astype(np.int16)
            nn = int(lv.sum())
            specs.append(oracle.PageSpec(oracle.PAGE_DATA, oracle.level_encode(lv, 1) + bytes([3]) + _run(nn, entry, 3),
                                         n, oracle.RLE_DICTIONARY))
        else:
            specs.append(oracle.PageSpec(oracle.PAGE_DATA, bytes([3]) + _run(n, entry, 3), n, oracle.RLE_DICTIONARY))
    got, ref = _check(oracle, ctx, specs, True, ptype=oracle.INT64, max_def=max_def)
    assert ref["status"] == 0 and set(np.unique(ref["values"])) == {dvals[4], dvals[0]}


def test_rle_boolean_v2_page_of_one_run(oracle, ctx):
    """RLE booleans ([i32 length][hybrid, w = 1], decoding.rs:339-349) of a required column in a v2
    page: one run of true, one of false."""
    specs = [oracle.PageSpec(oracle.PAGE_DATA_V2, _v1(_run(n, v, 1)), n, oracle.RLE, def_len=0)
             for n, v in ((5000, 1), (4097, 0))]
    got, ref = _check(oracle, ctx, specs, True, ptype=oracle.BOOLEAN, max_def=0)
    assert ref["status"] == 0 and int(np.asarray(ref["values"]).sum()) == 5000


def test_three_pages_odd_offsets_and_alignments(oracle, ctx):
    """Three run-only pages of 4097, 1 and 4095 levels: the second and third pages' levels start at
    odd element offsets of the output. Then the same with 0..15 bytes after each run, which moves
    the value sections through all 16 byte alignments."""
    for pad in range(16):
        rng = np.random.default_rng(pad)
        junk = rng.integers(0, 256, pad, dtype=np.uint8).tobytes()
        specs = [_page(oracle, rng, _run(n, 1, 1) + junk, n, nvals=n) for n in (4097, 1, 4095)]
        _check(oracle, ctx, specs, True, what=pad)
    rng = np.random.default_rng(99)
    for mis in (1, 2, 7):  # and the payloads themselves off their 64-byte alignment
        specs = [_page(oracle, rng, _run(n, 1, 1), n) for n in (4097, 1, 4095)]
        _check(oracle, ctx, specs, True, misalign=mis, what=("misalign", mis))


def _mixed_pages(oracle, rng, max_def=1):
    """A run-only page, a sparse page (random levels: bit-packed runs, the segment walk), a dense
    one-bit page of mostly bit-packed groups (p_null 0.1: the chunk walks at max_def 1) and one of
    more levels per stream byte (p_null 0.03: long RLE runs between the groups, the window path)."""
    n = 100_000
    return [_page(oracle, rng, _run(n, max_def, _width(max_def)), n, max_def=max_def),
            _random_page(oracle, rng, n, 0.5, max_def), _random_page(oracle, rng, n, 0.1, max_def),
            _random_page(oracle, rng, n, 0.03, max_def), _page(oracle, rng, _run(777, 0, _width(max_def)), 777,
                                                              max_def=max_def)]


def test_mixed_paths_in_one_chunk(oracle, ctx):
    import pqgpu
    rng = np.random.default_rng(6)
    _check(oracle, ctx, _mixed_pages(oracle, rng), True)
    assert ctx.last_paths() & pqgpu.PATH_LEVEL_D1  # (the third page: the chunk walks)


# ------------------------------------------------------------------------------ batches, slots

class _Job:
    """One pqg_decode_chunks call of fixed-width PLAIN chunks (ptype, specs, max_def) in flight."""

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
            d_def = torch.empty(nlev + 8, dtype=torch.int16, device="cuda")
            d_val = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
            cols.append(pqgpu.Column(ptype, -1, max_def, 0))
            outs.append(pqgpu.Output(d_def.data_ptr(), None, d_val.data_ptr(), cap, None, 0, 0, 0, 0))
            self.keep.append((d_def, d_val))
        self.oa = ctx.decode_chunks_async(cols, self.d_blob.data_ptr(), len(blob), arrays, outs,
                                          torch.cuda.current_stream().cuda_stream)

    def check(self, oracle, what=""):
        """After the sync: every chunk against the oracle."""
        import pqgpu
        for k, (ptype, specs, max_def) in enumerate(self.chunks):
            ref = oracle.read_column(ptype, specs, max_def=max_def)
            assert ref["status"] == 0, ref["message"]
            d_def, d_val = self.keep[k]
            o = self.oa[k]
            assert o.num_levels == len(ref["def"]) and o.num_values == len(ref["values"]), (what, k)
            np.testing.assert_array_equal(d_def[:o.num_levels].cpu().numpy(), ref["def"], err_msg=f"{what} chunk {k}")
            got = d_val[:o.num_values * pqgpu.VALUE_SIZE[ptype]].cpu().numpy().tobytes()
            assert got == np.asarray(ref["values"]).tobytes(), (what, k)


def test_mixed_paths_in_a_batch_of_two_widths(oracle, ctx):
    """The mixed chunk and a second chunk of def bit width 2 (run-only, random and run-only pages)
    in one pqg_decode_chunks: one pass of every kernel over both."""
    import pqgpu
    rng = np.random.default_rng(7)
    wide = [_page(oracle, rng, _run(4097, 3, 2), 4097, max_def=3, ptype=oracle.INT64),
            _random_page(oracle, rng, 30_000, 0.4, 3, ptype=oracle.INT64),
            _page(oracle, rng, _run(1 << 20, 1, 2), 4095, max_def=3, ptype=oracle.INT64, nvals=0)]
    job = _Job(ctx, [(oracle.INT32, _mixed_pages(oracle, rng), 1), (oracle.INT64, wide, 3)])
    st = ctx.sync_detail()
    assert st[0] == 0, (st, ctx.error_message())
    assert ctx.last_paths() & pqgpu.PATH_LEVEL_RUNS
    job.check(oracle)


@pytest.mark.parametrize("overlap", [1, 2])
def test_overlap_modes(oracle, ctx, overlap):
    """The speculative PLAIN copy beside the level decode (pqg_ctx_set_overlap 1, 2) on run-only
    INT32 pages: all present (the copy's offsets are right), all null and mixed with a random page."""
    rng = np.random.default_rng(8 + overlap)
    specs = [_page(oracle, rng, _run(4097, 1, 1), 4097), _page(oracle, rng, _run(1000, 0, 1), 1000),
             _random_page(oracle, rng, 20_000, 0.3), _page(oracle, rng, _run(4095, 1, 1), 4095)]
    ctx.set_overlap(overlap)
    try:
        _check(oracle, ctx, specs, True, what=overlap)
    finally:
        ctx.set_overlap(0)


# ------------------------------------------------------------------------------ the path is not taken

# def streams of 100 one-bit levels whose first header is not a run of >= 100 levels the fast parse takes
_NOT_TAKEN = {
    "count_0_then_run": _run(0, 1, 1) + _run(100, 1, 1),
    "count_0_alone": _run(0, 1, 1),
    "short_run_then_rle": _run(50, 1, 1) + _run(50, 0, 1),
    "short_run_then_bit_packed": _run(48, 1, 1) + _bp(7, bytes([0xFF] * 7)),  # 56 bit-packed levels of 1
    "short_run_then_eof": _run(50, 1, 1),
    "value_wider_than_w": _run(100, 2, 1),
    "varint_cut": b"\x80",
    "varint_cut_2": b"\xC8\x80",
    "value_byte_missing": _varint(200),  # the header of a run of 100, and the stream ends
    "five_byte_varint": _varint(1 << 29) + b"\x01",  # a run of 2^28: the reference reads it, the fast parse not
}


@pytest.mark.parametrize("case", sorted(_NOT_TAKEN))
def test_first_header_not_a_covering_run(oracle, ctx, case):
    """First headers the rule refuses, as a chunk of their own and as the second of three pages:
    the bit stays clear and the result, or the reference's error and its page, is the oracle's.

    count_0_alone, short_run_then_eof, varint_cut and varint_cut_2 are def streams that end before
    the page's levels: the reference's level decoder returns a short batch, read_batch then makes
    no progress and loops forever (HANG), which k_lv_fallback reports for columns without rep
    levels."""
    rng = np.random.default_rng(len(case))
    stream = _NOT_TAKEN[case]
    n = 100
    bad = _page(oracle, rng, stream, n)
    _check(oracle, ctx, [bad], False, what=case)
    _check(oracle, ctx, [_random_page(oracle, rng, 5000, 0.5), bad, _random_page(oracle, rng, 300, 0.5)], False,
           what=case)


def test_bit_packed_level_encoding(oracle, ctx):
    """A v1 page whose def levels are BIT_PACKED-encoded (levels.rs:203-209): no run headers at
    all, whatever its first bytes look like (all zero here: an RLE header of count 0; and 0xC8: one
    of count 100)."""
    rng = np.random.default_rng(11)
    n = 100
    for first in (0x00, 0xC8):
        spec = oracle.PageSpec(oracle.PAGE_DATA, bytes([first] * 13) + _values(oracle, rng, oracle.INT32, n), n,
                               oracle.PLAIN, def_encoding=oracle.BIT_PACKED)
        _check(oracle, ctx, [spec], False, what=first)
    lv = rng.integers(0, 2, n).astype(np.int16)
    lev = oracle.level_encode(lv, 1, encoding=oracle.BIT_PACKED)
    body = _values(oracle, rng, oracle.INT32, n)
    spec = oracle.PageSpec(oracle.PAGE_DATA, lev + body, n, oracle.PLAIN, def_encoding=oracle.BIT_PACKED)
    _check(oracle, ctx, [spec], False)


# ------------------------------------------------------------------------------ errors on the path

@pytest.mark.parametrize("cut", [1, 4, 5, 4000])
def test_value_section_too_short(oracle, ctx, cut):
    """An all-present run-only page (the second of three) whose value section holds fewer than n
    values: the reference's status (eof_err!, decoding.rs:138-186) on that page."""
    rng = np.random.default_rng(cut)
    specs = [_page(oracle, rng, _run(n, 1, 1), n) for n in (3000, 1000, 50)]
    specs[1] = oracle.PageSpec(specs[1].page_type, specs[1].buf[:-cut], 1000, oracle.PLAIN)
    got, ref = _check(oracle, ctx, specs, True, what=cut)
    assert ref["status"] != 0 and got["page"] == 1


# ------------------------------------------------------------------------------ tables that outlive a decode

def test_stale_tables_between_decodes(oracle, ctx):
    """One context: a sparse page of three segments, a run-only page of the same size, the sparse
    page again. The level tables (segments, run lists, page counts) outlive a decode; none of the
    earlier decode's may be read."""
    rng = np.random.default_rng(12)
    n = 300_000
    sparse = [_random_page(oracle, rng, n, 0.5)]
    assert int.from_bytes(sparse[0].buf[:4], "little") > 2 * 16384  # the def stream: three segments of 16 KiB
    runs = [_page(oracle, rng, _run(n, 1, 1), n)]
    for specs, taken in ((sparse, False), (runs, True), (sparse, False), (runs, True)):
        _check(oracle, ctx, specs, taken)


def test_alternating_batches_use_both_slots(oracle, ctx):
    """Two different batches enqueued alternately without a sync between them (the context's two
    slots), three rounds: run-only pages in one, random pages of other sizes in the other."""
    import pqgpu
    rng = np.random.default_rng(13)
    a = [(oracle.INT32, [_page(oracle, rng, _run(n, v, 1), n) for n, v in ((4097, 1), (1, 0), (4095, 1))], 1)]
    b = [(oracle.INT64, [_random_page(oracle, rng, 40_000, 0.5, 3, ptype=oracle.INT64),
                         _random_page(oracle, rng, 999, 0.1, 3, ptype=oracle.INT64)], 3),
         (oracle.INT32, [_random_page(oracle, rng, 20_000, 0.1)], 1)]
    for rnd in range(3):
        ja = _Job(ctx, a)
        jb = _Job(ctx, b)
        st = ctx.sync_detail()
        assert st[0] == 0, (rnd, st, ctx.error_message())
        assert not ctx.last_paths() & pqgpu.PATH_LEVEL_RUNS  # (the last decode's: b)
        ja.check(oracle, ("a", rnd))
        jb.check(oracle, ("b", rnd))
        jb2 = _Job(ctx, b)
        ja2 = _Job(ctx, a)
        st = ctx.sync_detail()
        assert st[0] == 0, (rnd, st, ctx.error_message())
        assert ctx.last_paths() & pqgpu.PATH_LEVEL_RUNS  # (a)
        jb2.check(oracle, ("b2", rnd))
        ja2.check(oracle, ("a2", rnd))
