"""CPU: what the builders of deflate_inputs.py promise (a later edit must not quietly defuse an input), the restated token parse against host zlib's
Z_RLE parse, and the block walker of inflate_walk.py against zlib."""
import zlib

import numpy as np
import pytest

import deflate_inputs as di
from inflate_walk import walk


def _zrle(b):
    c = zlib.compressobj(4, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(b) + c.flush()


BUILDERS = {
    "deep_literal_code": di.deep_literal_code,
    "deep_code_length_code": di.deep_code_length_code,
    "run_table": di.run_table,
    "ff_segment": lambda: di.one_byte_segment(0xFF),
    "zero_segment": lambda: di.one_byte_segment(0),
    "every_symbol": di.every_symbol,
    "high_bytes": lambda: di.high_bytes(40000, 1),
    "noise": lambda: di.noise(40000, 1),
    "high_bytes_3": lambda: di.high_bytes(3, 0),
    "noise_1": lambda: di.noise(1, 0),
}
SEGMENTS = {"run_table": 3, "high_bytes": 3, "noise": 3}                 # every other builder is one segment at the most


def test_deep_literal_code_needs_the_15_bit_limiter():
    x = di.deep_literal_code()
    assert x.dtype == np.uint8 and len(x) == 10944 and np.all(x[1:] != x[:-1])
    hist = di.tokens(x)
    assert sorted(hist[hist > 0]) == sorted([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181])
    assert di.huffman_depths(hist).max() == 18
    lens, deepest = di.limited_lengths(hist, 15)
    assert deepest == 18
    assert sorted(lens[hist > 0]) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 15, 15, 15, 15, 15]


def test_deep_code_length_code_needs_the_7_bit_limiter():
    x = di.deep_code_length_code()
    assert x.dtype == np.uint8 and len(x) <= di.SEG and np.all(x[1:] != x[:-1])
    lens, deepest = di.limited_lengths(di.tokens(x), 15)
    assert deepest <= 15                                                # this input is about the other limiter
    clh = di.code_length_histogram(lens)
    assert clh.sum() == len(di.code_length_sequence(lens)) and clh[1] >= 1
    heap, own = di.code_length_code_depths(x)
    print("code-length histogram", clh.tolist(), "depth by heap", heap, "by the encoder's algorithm", own)
    assert heap >= 8 and own >= 8
    cl, _ = di.limited_lengths(clh, 7)
    assert cl.max() == 7 and sum(2.0 ** -int(n) for n in cl if n) == 1.0


def test_the_seeded_search_finds_the_committed_draw():
    assert di.search_deep_code_length_code(di.CL_SEED, di.CL_DRAW + 1) == di.CL_DRAW


def test_limited_lengths_are_optimal_where_no_limit_binds():
    rng = np.random.default_rng(0)
    for n in (2, 3, 19, 286):
        hist = rng.integers(0, 50, n) * (rng.random(n) < 0.7)
        hist[0] = hist[1] = 7
        lens, deepest = di.limited_lengths(hist, 63)
        assert deepest == lens.max() and np.all((lens > 0) == (hist > 0))
        assert sum(2.0 ** -int(v) for v in lens if v) == 1.0
        assert (lens * hist).sum() == (di.huffman_depths(hist) * hist).sum()       # both are minimum-redundancy codes


def test_run_table_covers_every_remainder_at_every_offset_and_both_edges():
    x = di.run_table()
    start, n, v = di.runs(x)
    assert np.all(v[1:] != v[:-1])
    inside = start // di.SEG == (start + n - 1) // di.SEG                # runs that no segment edge cuts
    q, r = np.divmod(n[inside] - 1, 258)
    seen = set(zip(q.tolist(), r.tolist(), (start[inside] % di.SPAN).tolist()))
    assert {(a, b, c) for a in di.RUN_Q for b in di.RUN_R for c in di.RUN_OFF} <= seen
    ends = (start + n).tolist()
    assert any(s <= 16380 and e == 16391 for s, e in zip(start.tolist(), ends))                # the run over bytes 16 380..16 390
    assert any(e == 2 * di.SEG and m >= 259 for e, m in zip(ends, n.tolist()))                 # a run that ends exactly at a segment edge
    assert any(e % di.SPAN == 0 and m >= 2 for e, m in zip(ends, n.tolist()))                  # and runs that end at a span edge
    assert 2 * di.SEG < len(x) <= 3 * di.SEG
    assert x[di.SEG - 1] == x[di.SEG] and x[2 * di.SEG - 1] != x[2 * di.SEG]


def test_every_symbol_uses_all_286_symbols():
    x = di.every_symbol()
    hist = di.tokens(x)
    assert len(hist) == 286 and np.all(hist > 0)
    assert di.limited_lengths(hist, 15)[0][285] > 0


def test_one_byte_segment_is_a_literal_and_matches():
    for v in (0, 0xFF):
        x = di.one_byte_segment(v)
        assert len(x) == di.SEG and np.all(x == v)
        assert di.token_list(x) == [v] + [(258, 1)] * 63 + [(129, 1)]


def test_high_bytes_and_noise():
    h, z = di.high_bytes(di.SEG, 3), di.noise(di.SEG, 3)
    assert h.min() == 0xF0 and h.max() == 0xFF and len(np.unique(z)) == 256
    assert np.array_equal(h, di.high_bytes(di.SEG, 3)) and not np.array_equal(h, di.high_bytes(di.SEG, 4))
    assert len(_zrle(h.tobytes())) < 0.6 * di.SEG and len(_zrle(z.tobytes())) > di.SEG


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_builder_size_and_host_round_trip(name):
    x = BUILDERS[name]()
    assert x.dtype == np.uint8 and x.ndim == 1
    assert len(di.segments(x)) == SEGMENTS.get(name, 1)
    assert zlib.decompress(zlib.compress(x.tobytes())) == x.tobytes()
    for seg in di.segments(x):
        toks = di.token_list(seg)
        hist = np.zeros(286, np.int64)
        for t in toks:
            hist[t if isinstance(t, int) else di.length_symbol(t[0])] += 1
        hist[256] += 1
        assert np.array_equal(hist, di.tokens(seg))
        assert sum(1 if isinstance(t, int) else t[0] for t in toks) == len(seg)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_walker_equals_zlib_on_host_rle_streams(name):
    x = BUILDERS[name]().tobytes()
    for stream in (_zrle(x), zlib.compress(x, 1), zlib.compress(x, 9)):
        out, blocks = walk(stream, keep_tokens=True)
        assert out == zlib.decompress(stream) == x
        assert sum(b["nbytes"] for b in blocks) == len(x) and [b["bfinal"] for b in blocks] == [0] * (len(blocks) - 1) + [1]
        assert blocks[0]["bit_start"] == 16 and all(a["bit_end"] == b["bit_start"] for a, b in zip(blocks, blocks[1:]))
        for b in blocks:
            assert sum(1 if isinstance(t, int) else t[0] for t in b["tokens"]) == b["nbytes"]
            if b["btype"] == 2:
                assert 257 <= b["hlit"] == len(b["ll_lengths"]) <= 286 and 4 <= b["hclen"] <= 19 and len(b["cl_lengths"]) == 19
                assert sum(2.0 ** -n for n in b["ll_lengths"] if n) == 1.0 and max(b["cl_lengths"]) <= 7
    out, blocks = walk(_zrle(x), keep_tokens=True)
    assert all(b["distances"] <= {1} for b in blocks)
    if len(x) <= di.SEG:                                                # host Z_RLE parses a run as the encoder's contract states it
        assert [t for b in blocks for t in b["tokens"]] == di.token_list(np.frombuffer(x, np.uint8))


def test_walker_rejects_what_zlib_rejects():
    good = _zrle(di.every_symbol().tobytes() * 9)                        # (a dynamic block)
    assert walk(good)[1][0]["btype"] == 2
    bad_sum = good[:-1] + bytes([good[-1] ^ 1])
    for bad in (bad_sum, good + b"\0", good[:-5], b"\x78\x02" + good[2:], good[:2] + bytes([good[2] | 6]) + good[3:]):
        with pytest.raises(ValueError):
            walk(bad)
    for bad in (bad_sum, good[:-5], good[:2] + bytes([good[2] | 6]) + good[3:]):
        with pytest.raises(zlib.error):
            zlib.decompress(bad)
    d = zlib.decompressobj()
    d.decompress(good + b"\0")
    assert d.unused_data == b"\0"
