"""A deflate block walker in plain Python: inflates a zlib stream (RFC 1950 / 1951) and reports what zlib does not -- one record per block, so that a
test can show which path of an encoder a stream took.  walk(stream) -> (bytes, blocks); each block is a dict:
    bfinal, btype           the block header
    bit_start, bit_end      bit offsets in the stream (the zlib header is bits 0..15)
    nbytes                  bytes the block produced
    hlit, hclen             the counts a dynamic block declares (257..286, 4..19), else None
    ll_lengths, cl_lengths  code length per literal/length symbol and per code-length symbol of a dynamic block (0: unused), else None
    distances               the set of match distances seen
    tokens                  with keep_tokens: literals as byte values and matches as (length, distance), in stream order
Malformed input raises ValueError: a bad header, an over-subscribed code, an incomplete code of more than one symbol, an unassigned code in the data, a
distance before the start, a stored block whose lengths disagree, a wrong Adler-32, bytes after the checksum."""
import zlib

_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_tables = {}


def _table(lengths):
    """code lengths -> (lookup by the next `bits` stream bits -> symbol << 4 | length, or 0 for an unassigned code; bits)"""
    key = tuple(lengths)
    if key in _tables:
        return _tables[key]
    bits = max(lengths)
    if bits == 0:
        raise ValueError("a code without symbols")
    count = [0] * (bits + 1)
    for n in lengths:
        count[n] += 1
    count[0] = 0
    kraft = sum(c << (bits - n) for n, c in enumerate(count) if n)
    if kraft > 1 << bits or (kraft < 1 << bits and sum(count) != 1):
        raise ValueError("over-subscribed or incomplete code")
    code, first = 0, [0] * (bits + 1)
    for n in range(1, bits + 1):
        code = (code + count[n - 1]) << 1
        first[n] = code
    tab = [0] * (1 << bits)
    for s, n in enumerate(lengths):
        if n:
            rev = int(format(first[n], "0%db" % n)[::-1], 2)          # Huffman codes travel most significant bit first
            first[n] += 1
            tab[rev::1 << n] = [s << 4 | n] * (1 << (bits - n))
    if len(_tables) > 64:
        _tables.clear()
    _tables[key] = tab, bits
    return tab, bits


def walk(stream, keep_tokens=False):
    data = bytes(stream)
    if len(data) < 6 or data[0] & 15 != 8 or data[0] >> 4 > 7 or (data[0] << 8 | data[1]) % 31 or data[1] & 32:
        raise ValueError("not a zlib stream without a dictionary")
    end = len(data) - 4
    data += bytes(8)                                                    # the refill below reads four bytes at a time
    pos, buf, cnt = 2, 0, 0                                             # next byte to load; loaded bits; how many
    out, blocks = bytearray(), []
    while True:
        if cnt < 32:
            buf |= int.from_bytes(data[pos:pos + 4], "little") << cnt; pos += 4; cnt += 32
        blk = dict(bfinal=buf & 1, btype=buf >> 1 & 3, bit_start=8 * pos - cnt, hlit=None, hclen=None, ll_lengths=None, cl_lengths=None,
                   distances=set(), tokens=[] if keep_tokens else None)
        buf >>= 3; cnt -= 3
        start, toks, dists = len(out), blk["tokens"], blk["distances"]
        if blk["btype"] == 3:
            raise ValueError("block type 3")
        if blk["btype"] == 0:
            pos -= cnt // 8; buf = cnt = 0                              # drop the bits up to the byte boundary, unread the whole bytes
            n = data[pos] | data[pos + 1] << 8
            if n ^ 0xFFFF != data[pos + 2] | data[pos + 3] << 8 or pos + 4 + n > end:
                raise ValueError("stored block: bad lengths")
            out += data[pos + 4:pos + 4 + n]
            if keep_tokens:
                toks.extend(data[pos + 4:pos + 4 + n])
            pos += 4 + n
        else:
            if blk["btype"] == 1:
                ll, dl = _FIXED_LL, [5] * 32
            else:
                hlit, hdist, hclen = 257 + (buf & 31), 1 + (buf >> 5 & 31), 4 + (buf >> 10 & 15)
                buf >>= 14; cnt -= 14
                if hlit > 286 or hdist > 30:
                    raise ValueError("too many length or distance codes")
                cl = [0] * 19
                for k in range(hclen):
                    if cnt < 32:
                        buf |= int.from_bytes(data[pos:pos + 4], "little") << cnt; pos += 4; cnt += 32
                    cl[_CLORDER[k]] = buf & 7; buf >>= 3; cnt -= 3
                tab, bits = _table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    if cnt < 32:
                        buf |= int.from_bytes(data[pos:pos + 4], "little") << cnt; pos += 4; cnt += 32
                    e = tab[buf & (1 << bits) - 1]
                    if not e:
                        raise ValueError("unassigned code-length code")
                    buf >>= e & 15; cnt -= e & 15
                    s = e >> 4
                    if s < 16:
                        lens.append(s); continue
                    if s == 16 and not lens:
                        raise ValueError("repeat without a previous length")
                    xb, base, v = ((2, 3, lens[-1]) if s == 16 else (3, 3, 0) if s == 17 else (7, 11, 0))
                    lens += [v] * (base + (buf & (1 << xb) - 1)); buf >>= xb; cnt -= xb
                if len(lens) > hlit + hdist or lens[256] == 0:
                    raise ValueError("code lengths overrun, or no end-of-block code")
                ll, dl = lens[:hlit], lens[hlit:]
                blk.update(hlit=hlit, hclen=hclen, ll_lengths=ll, cl_lengths=cl)
            ltab, lbits = _table(ll)
            dtab, dbits = _table(dl) if any(dl) else (None, 0)
            lmask, dmask = (1 << lbits) - 1, (1 << dbits) - 1
            while True:
                if cnt < 32:
                    if pos > end + 8:
                        raise ValueError("the stream ends inside a block")
                    buf |= int.from_bytes(data[pos:pos + 4], "little") << cnt; pos += 4; cnt += 32
                e = ltab[buf & lmask]
                n = e & 15; buf >>= n; cnt -= n
                s = e >> 4
                if s < 256:
                    if not e:
                        raise ValueError("unassigned literal/length code")
                    out.append(s)
                    if keep_tokens:
                        toks.append(s)
                    continue
                if s == 256:
                    break
                if s > 285 or dtab is None:
                    raise ValueError("length symbol beyond 285, or a match without a distance code")
                xb = _LEXT[s - 257]
                length = _LBASE[s - 257] + (buf & (1 << xb) - 1); buf >>= xb; cnt -= xb
                if cnt < 32:
                    buf |= int.from_bytes(data[pos:pos + 4], "little") << cnt; pos += 4; cnt += 32
                e = dtab[buf & dmask]
                if not e or e >> 4 > 29:
                    raise ValueError("unassigned distance code")
                buf >>= e & 15; cnt -= e & 15
                xb = _DEXT[e >> 4]
                dist = _DBASE[e >> 4] + (buf & (1 << xb) - 1); buf >>= xb; cnt -= xb
                if dist > len(out):
                    raise ValueError("distance before the start of the data")
                if dist == 1:
                    out += out[-1:] * length
                else:
                    for _ in range(length):
                        out.append(out[-dist])
                dists.add(dist)
                if keep_tokens:
                    toks.append((length, dist))
        blk.update(bit_end=8 * pos - cnt, nbytes=len(out) - start)
        if blk["bit_end"] > 8 * end:
            raise ValueError("the stream ends inside a block")
        blocks.append(blk)
        if blk["bfinal"]:
            break
    at = pos - cnt // 8
    if at != end:
        raise ValueError("%d bytes between the last block and the checksum" % (end - at))
    if int.from_bytes(data[end:end + 4], "big") != zlib.adler32(out):
        raise ValueError("wrong Adler-32")
    return bytes(out), blocks
