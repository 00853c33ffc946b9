"""The device deflate encoder (csrc/iris_deflate.h, png_chunk_kernel / png_emit_kernel of csrc/iris_png.h) on the byte streams of deflate_inputs.py:
both length limiters, run remainders and edges, streams of more than 256 segments, unaligned and odd-length sources.  The reference is host zlib
(a stream must inflate to its input, end there and carry the right Adler-32); the block walker of inflate_walk.py shows that the path a case aims
at was taken.  No tolerance anywhere: equalities and the hard bounds of the format.

Every stream: one non-empty block per 16 KiB segment, only the last with BFINAL, every distance 1.  A non-final DYNAMIC segment is followed by an
empty stored block that ends byte-aligned (the sync flush), so a stream of dynamic segments only has 2 * segments - 1 blocks; a STORED segment ends
byte-aligned by itself and the encoder adds nothing after it (the stream bound, 5 bytes a segment, leaves no room for more).

Stream sizes against host zlib's Z_RLE at level 4 (printed by the tests, measured on an MI355X; a length-limited code need not match zlib's):
    deep_literal_code        3 626 bytes against  3 627: 0.9997   (lengths 1..12, 14 and six of 15, as zlib limits them)
    deep_code_length_code    8 842 bytes against  8 843: 0.9999   (code-length code lengths 1, 2, 4, 4, 5, 5 and eight of 7)
    run_table               10 664 bytes against 10 651: 1.0012   (three blocks and two sync flushes against one block)
    one_byte_segment(0xFF)      38 bytes against     38: 1.0000
    one_byte_segment(0)         38 bytes against     38: 1.0000
    every_symbol               368 bytes against    358: 1.0279   (host zlib chooses a fixed-code block here, which this encoder never writes)"""
import struct
import zlib

import numpy as np
import pytest

import deflate_inputs as di
from inflate_walk import walk

pytestmark = pytest.mark.gpu


def _zrle(b):
    c = zlib.compressobj(4, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(b) + c.flush()


def _encode_once(rows):
    import torch
    from iris_amd import _lib as L
    lib = L.lib()
    M, n = rows.shape
    cap, ws_bytes = int(lib.iris_png_stream_bound(n)), int(lib.iris_png_workspace_bytes(M, n))
    assert ws_bytes > 0
    streams = torch.zeros(M * cap, dtype=torch.uint8, device=rows.device)
    offs = torch.zeros(M + 1, dtype=torch.int64, device=rows.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=rows.device)
    L.check(lib.iris_png_encode(L.ptr(rows), M, n, L.ptr(streams), L.ptr(offs), L.ptr(ws), ws_bytes, L.stream()))
    torch.cuda.synchronize()
    offs = offs.cpu().numpy()
    assert offs[0] == 0 and np.all(np.diff(offs) > 0) and offs[M] <= M * cap
    host = streams[:int(offs[M])].cpu().numpy()
    return [host[offs[m]:offs[m + 1]].tobytes() for m in range(M)]


def device_zlib(buffers, addresses=None):
    """M uint8 arrays of equal length -> their M bare zlib streams from iris_png_encode, encoded twice (the second encode returns the same bytes).
    addresses: a list that receives each source's device address."""
    import torch
    rows = torch.from_numpy(np.stack([np.asarray(b, np.uint8) for b in buffers])).cuda()
    if addresses is not None:
        addresses += [rows.data_ptr() + m * rows.shape[1] for m in range(rows.shape[0])]
    first, second = _encode_once(rows), _encode_once(rows)
    assert first == second
    return first


def _bound(n):
    from iris_amd import _lib as L
    return int(L.lib().iris_png_stream_bound(n))


def check_stream(s, x, keep_tokens=False):
    """The checks every stream has to pass -> the walker's record of each segment's block"""
    x = np.asarray(x, np.uint8)
    d = zlib.decompressobj()
    assert d.decompress(s) == x.tobytes() and d.eof and d.unused_data == b""
    assert len(s) <= _bound(len(x)) == len(x) + 5 * -(-len(x) // di.SEG) + 6
    out, blocks = walk(s, keep_tokens)
    assert out == x.tobytes()
    segs, per_seg, k = di.segments(x), [], 0
    for i, seg in enumerate(segs):
        b, last = blocks[k], i == len(segs) - 1
        assert b["btype"] in (0, 2) and b["nbytes"] == len(seg) and b["bfinal"] == int(last) and b["distances"] <= {1}, (i, b["btype"], b["nbytes"])
        k += 1
        if b["btype"] == 2 and not last:                                 # the sync flush
            e = blocks[k]
            assert (e["btype"], e["nbytes"], e["bfinal"], e["bit_end"] % 8) == (0, 0, 0, 0), i
            k += 1
        assert blocks[k - 1]["bit_end"] % 8 == 0 or last, i              # the stream is the concatenation of its segments
        per_seg.append(b)
    assert k == len(blocks)
    if all(b["btype"] == 2 for b in per_seg):
        assert len(blocks) == 2 * len(segs) - 1
    return per_seg


def _kraft_is_one(lengths):
    return sum(1 << (15 - n) for n in lengths if n) == 1 << 15


def _report(name, s, x):
    host = _zrle(np.asarray(x, np.uint8).tobytes())
    print(f"{name}: {len(x)} bytes -> device {len(s)}, host Z_RLE {len(host)}, ratio {len(s) / len(host):.4f}")


def test_literal_code_deeper_than_15_bits_is_limited_to_a_complete_code():
    x = di.deep_literal_code()
    hist = di.tokens(x)
    assert di.huffman_depths(hist).max() == 18
    (s,) = device_zlib([x])
    (b,) = check_stream(s, x)
    _report("deep_literal_code", s, x)
    lens = np.array(b["ll_lengths"] + [0] * (286 - b["hlit"]))
    print("literal/length code lengths", sorted(lens[lens > 0].tolist()))
    assert b["btype"] == 2 and lens.max() == 15 and _kraft_is_one(lens)
    assert np.array_equal(lens > 0, hist > 0)
    used = np.flatnonzero(hist)
    order = used[np.argsort(hist[used], kind="stable")]
    for a, c in zip(order, order[1:]):                                   # a symbol with a higher count never has a longer code
        assert hist[a] == hist[c] or lens[a] >= lens[c], (a, c)


def test_code_length_code_deeper_than_7_bits_is_limited_to_a_complete_code():
    x = di.deep_code_length_code()
    assert min(di.code_length_code_depths(x)) >= 8
    (s,) = device_zlib([x])
    (b,) = check_stream(s, x)
    _report("deep_code_length_code", s, x)
    print("code-length code lengths", b["cl_lengths"], "HCLEN", b["hclen"])
    assert b["btype"] == 2 and max(b["cl_lengths"]) == 7 and _kraft_is_one(b["cl_lengths"])
    assert max(b["ll_lengths"]) <= 15 and _kraft_is_one(b["ll_lengths"])


@pytest.mark.parametrize("name", ["run_table", "ff_segment", "zero_segment", "every_symbol"])
def test_tokens_are_the_contracts_parse(name):
    x = {"run_table": di.run_table, "ff_segment": lambda: di.one_byte_segment(0xFF), "zero_segment": lambda: di.one_byte_segment(0),
         "every_symbol": di.every_symbol}[name]()
    (s,) = device_zlib([x])
    blocks = check_stream(s, x, keep_tokens=True)
    _report(name, s, x)
    assert len(blocks) == {"run_table": 3}.get(name, 1)
    for i, (b, seg) in enumerate(zip(blocks, di.segments(x))):
        assert b["btype"] == 2, i
        assert b["tokens"] == di.token_list(seg), i                      # (a run that crosses a segment edge restarts with a literal)
        assert _kraft_is_one(b["ll_lengths"]) and _kraft_is_one(b["cl_lengths"])
    if name == "run_table":
        assert blocks[1]["tokens"][:2] == [int(x[di.SEG]), (6, 1)] and x[di.SEG - 1] == x[di.SEG]
    if name == "every_symbol":
        assert blocks[0]["hlit"] == 286


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 32768, 32769])
def test_sizes_and_unaligned_sources(n):
    bufs, addr = [di.high_bytes(n, n), di.noise(n, n), di.run_table()[:n]], []
    streams = device_zlib(bufs, addr)
    kinds = [[b["btype"] for b in check_stream(s, x)] for s, x in zip(streams, bufs)]
    print(n, [a % 4 for a in addr], kinds)
    assert addr[0] % 4 == 0
    if n >= 16383:
        whole = max(1, n // di.SEG)                                      # (a last segment of one byte may be stored whatever it holds)
        assert set(kinds[0][:whole]) == {2} and kinds[2][0] == 2 and set(kinds[1][:whole]) == {0}
        if n % 2:                                                        # a source that is not 4-byte aligned and compresses dynamically
            assert addr[1] % 4 != 0 and addr[2] % 4 == 2


@pytest.mark.parametrize("n", [256 * di.SEG + 1, 513 * di.SEG - 7])
def test_more_than_256_segments(n):
    nseg = -(-n // di.SEG)
    assert nseg in (257, 513)
    ff, a = di.one_byte_segment(0xFF), di.noise(n, 7)
    for k in range(0, nseg, 2):
        a[k * di.SEG:(k + 1) * di.SEG] = ff[:len(a[k * di.SEG:(k + 1) * di.SEG])]
    b = di.high_bytes(n, 8)
    sa, sb = device_zlib([a, b])
    ba, bb = check_stream(sa, a), check_stream(sb, b)
    print(n, "segments", len(ba), len(bb), "stream bytes", len(sa), len(sb))
    assert len(ba) == len(bb) == nseg
    full = n // di.SEG
    assert [k["btype"] for k in ba[:full]] == [2, 0] * (full // 2) + [2] * (full % 2)      # dynamic and stored blocks alternate in A
    assert all(k["btype"] == 2 for k in bb[:full])


def _records(buf):
    out, o, buf = [], 0, bytes(buf)
    while o < len(buf):
        y, size = struct.unpack_from("<ii", buf, o)
        out.append((y, buf[o + 8:o + 8 + size]))
        o += 8 + size
    assert o == len(buf)
    return out


@pytest.mark.parametrize("T", [0, 1, 5])
@pytest.mark.parametrize("B", [16385, 12289 + 2])
def test_exr_records_of_hand_made_blocks(B, T):
    import torch
    from iris_amd.utils import exr
    take = lambda x: np.resize(x, B)                                     # noqa: E731  (a prefix, or the input repeated up to B bytes)
    kinds = [["noise", "runs", "deep"], ["runs", "noise", "noise"]]
    make = {"noise": lambda i: di.noise(B, 10 + i), "runs": lambda i: take(di.run_table()), "deep": lambda i: take(di.deep_literal_code())}
    full_h = np.stack([np.stack([make[k](3 * m + i) for i, k in enumerate(row)]) for m, row in enumerate(kinds)])
    tail_h = np.stack([di.noise(T, 20), di.high_bytes(T, 21)]) if T else np.zeros((2, 0), np.uint8)
    full, tail = torch.from_numpy(full_h).cuda(), torch.from_numpy(tail_h).cuda()
    n_raw = n_z = n_raw_unaligned = 0
    for comp, lines in (("zip", 16), ("zips", 1)):
        rec, offs = exr.zip_encode_torch(full, tail, comp)
        rec2, offs2 = exr.zip_encode_torch(full, tail, comp)
        torch.cuda.synchronize()
        assert torch.equal(offs, offs2) and torch.equal(rec[:int(offs[-1])], rec2[:int(offs[-1])])
        rec, offs = rec.cpu().numpy(), offs.cpu().numpy()
        assert offs[0] == 0 and offs[-1] <= rec.shape[0] and np.all(np.diff(offs) > 0)
        for m in range(2):
            chunks = _records(rec[offs[m]:offs[m + 1]])
            preds = [(full_h[m, i], full.data_ptr() + (3 * m + i) * B, kinds[m][i]) for i in range(3)]
            preds += [(tail_h[m], tail.data_ptr() + m * T, "noise")] if T else []
            assert [y for y, _ in chunks] == [i * lines for i in range(len(preds))]
            for (y, data), (pred, address, kind) in zip(chunks, preds):
                if len(data) == len(pred):
                    assert kind == "noise", (m, y)
                    assert data == exr._unpredict(pred.tobytes()), (m, y, address % 4)
                    n_raw += 1
                    n_raw_unaligned += address % 4 != 0
                else:
                    assert kind != "noise" and len(data) < len(pred), (m, y)
                    blocks = check_stream(data, pred)
                    assert blocks[0]["btype"] == 2
                    n_z += 1
    assert n_raw > 0 and n_z > 0 and n_raw_unaligned > 0
