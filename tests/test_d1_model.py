"""The model of _d1model.py against the oracle, and every crafted stream of test_gpu_d1.py against
the model: a stream's name says which path it is to take, and here it proves that it does, so a GPU
test that passes has run the code it is about."""
import numpy as np
import pytest

import _d1model as M
import _d1streams as S


@pytest.mark.parametrize("name", sorted(S.BUILDERS))
def test_stream_is_what_its_name_says(oracle, name):
    c = S.case(oracle, name)
    # the model's chain reads the levels the reference reads (for a request past the stream's end too)
    for n in (c.n, c.n + 100_000):
        st, lv = oracle.rle_decode(c.stream, 1, n, type_size=2)
        if st == 0:
            assert len(lv) == M.levels(c.stream, n), (name, n)
    assert c.n <= 400_000
    if c.selected is not None:
        assert M.selected(c.stream, c.n, 1) == c.selected, name
    if c.cause is not None:
        why, pos = M.cause(c.stream, c.n)
        assert why in ((c.cause,) if isinstance(c.cause, str) else c.cause), (name, why, pos)
        # and the kernels' decisions, replayed: taken pages are not handed back, the others are,
        # at the site their cause means
        site = M.handback(c.stream, c.n)
        assert site == (None if why == "taken" else S.SITE_OF.get(name, S.SITE[why])), (name, why, site)


def test_model_levels_match_the_oracle_bit_for_bit(oracle):
    """The chain's kinds, values and payload offsets, not only its counts: levels rebuilt from the
    model's headers equal the oracle's."""
    for name in ("writer_p0.3_n20001", "zero_counts", "foreign_bp125", "bp3_segment", "dead5_first"):
        c = S.case(oracle, name)
        out = []
        for h in M.true_chain(c.stream):
            if h.kind == "rle":
                out.append(np.full(h.count, h.value, np.int16))
            else:
                pay = np.frombuffer(c.stream[h.value:h.value + h.count // 8], np.uint8)
                out.append(np.unpackbits(pay, bitorder="little").astype(np.int16))
        mine = np.concatenate(out)[:c.n]
        st, lv = oracle.rle_decode(c.stream, 1, c.n, type_size=2)
        assert st == 0
        np.testing.assert_array_equal(mine, lv, err_msg=name)


def test_selection_rule_edges(oracle):
    s = S.case(oracle, "writer_p0.1_n20001").stream
    assert M.selected(s, 20_001, 1) and not M.selected(s, 20_001, 2) and not M.selected(s, 0, 1)
    assert not M.selected(S.run(1 << 20, 1) + s, 20_001, 1)  # run-only: the plan settles it
    assert M.selected(S.run(20_000, 1) + s, 20_001, 1)  # a first run one level short is not
    assert [len(S.case(oracle, f"slen_{k}").stream) for k in (1087, 1088)] == [1087, 1088]
    for at in (1003, 1004):  # the 64th header begins there
        assert M.true_chain(S.case(oracle, f"probe_edge_{at}").stream)[63].pos == at
    for slen in S.LENGTHS:
        assert len(S.case(oracle, f"len{slen}_all").stream) == slen


def test_segments_and_rounds(oracle):
    """Writer pages of one, two and three segments; long runs spanning bitmap rounds; the foreign
    run that enters a segment off its start; hand-backs in the segment they are named for."""
    for p, n in S.WRITER:
        want = {20_001: 1, 130_003: 2, 300_007: 3}[n]
        assert M.segments(S.case(oracle, f"writer_p{p}_n{n}").stream) == want, (p, n)
    for name in ("long_run_140000_1", "long_run_300000_0"):
        c = S.case(oracle, name)
        acc = 0
        for h in M.true_chain(c.stream):
            if h.count >= 140_000:
                assert h.pos // M.SEG == 1 and acc % 32 != 0 and h.count > M.RB, name
            acc += h.count
    c = S.case(oracle, "foreign_bp100_segment")
    assert any(h.pos == M.SEG + 38 for h in M.true_chain(c.stream))
    for what in S.HANDBACK:
        for where, seg in (("first", 0), ("last", 2)):
            c = S.case(oracle, f"{what}_{where}")
            why, pos = M.cause(c.stream, c.n)
            seg = max(seg, 1) if what == "entry64" else seg  # (met where the chain enters the next segment)
            assert pos // M.SEG == seg and M.segments(c.stream) >= 2, (what, where, pos)
    why, pos = M.cause(S.case(oracle, "unknown").stream, 10 ** 9)
    assert (why, pos) == ("unknown", M.SEG + 40)
    c = S.case(oracle, "far_many")
    assert sum(1 for h in M.true_chain(c.stream) if h.next // 64 - h.pos // 64 >= 2) >= 5


def test_cause_on_plain_streams():
    assert M.cause(S.sparse(2000), 1000) == ("taken", None)
    assert M.cause(S.sparse(2000), 1001) == ("short", 2000)
    assert M.cause(S.sparse(100) + S.run(5, 3), 55)[0] == "value>1"
    assert M.cause(S.sparse(100) + S.run(5, 3), 50) == ("taken", None)  # the run is never read
    assert M.cause(S.sparse(100) + b"\x90\x80\x80\x80\x00\x01", 55) == ("dead", 100)
    assert M.cause(S.sparse(100) + b"\x7f" + b"\0" * 10, 900) == ("dead", 100)  # payload cut
    assert M.cause(S.sparse(62) + S.bp(64, bytes(64)) + S.sparse(100), 600) == ("far", 62)
    assert M.cause(S.sparse(64) + S.bp(64, bytes(64)) + S.sparse(100), 590) == ("taken", None)
    s = S.sparse(M.SEG - 10) + S.bp(160, bytes(160)) + S.sparse(100)
    assert M.cause(s, 9000) == ("taken", None) and M.cause(s, 9500) == ("entry>=64", M.SEG + 152)


def _def_stream(spec):
    """The first level stream of a v1 page: [i32 length][stream]."""
    k = int.from_bytes(spec.buf[:4], "little")
    return spec.buf[4:4 + k]


def test_neighbour_pages_of_the_gpu_tests(oracle):
    """The writer pages test_gpu_d1.py puts around a case are selected and taken themselves (its
    assertions on the bits count on it); its window-path page (p_null 0.03) is not selected; the
    rep-level pages' streams are; and beside a cut def stream the whole rep stream is."""
    for seed in range(1, 10):
        a, _, b = S.around(oracle, None, seed)
        for spec in (a, b):
            s = _def_stream(spec)
            assert M.selected(s, spec.num_values, 1) and M.handback(s, spec.num_values) is None, seed
    w = S.random_page(oracle, np.random.default_rng(70), 50_001, 0.03)
    assert not M.selected(_def_stream(w), w.num_values, 1) and M.probe_dense(_def_stream(w))
    for max_def in (2, 1):  # the rep-level pages: the rep stream, and at max_def 1 the def stream too
        rng = np.random.default_rng(60 + max_def)
        for n in (20_001, 130_003, 9_001):
            spec = S.rep_page(oracle, rng, n, max_def)
            rep = _def_stream(spec)
            assert M.selected(rep, n, 1) and M.handback(rep, n) is None, (max_def, n)
            if max_def == 1:
                d = spec.buf[4 + len(rep):]
                d = d[4:4 + int.from_bytes(d[:4], "little")]
                assert M.selected(d, n, 1) and M.handback(d, n) is None, n
    for name in S.SHORT_CASES:
        for three in (False, True):
            for spec in S.short_rep_pages(oracle, name, three):
                rep = _def_stream(spec)
                assert M.selected(rep, spec.num_values, 1) and M.handback(rep, spec.num_values) is None, name
            bad = S.short_rep_pages(oracle, name, three)[int(three)]
            d = bad.buf[4 + len(_def_stream(bad)):]
            assert d[4:4 + int.from_bytes(d[:4], "little")] == S.case(oracle, name).stream
