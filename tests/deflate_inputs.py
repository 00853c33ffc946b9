"""Byte streams aimed at the paths of the device deflate encoder (csrc/iris_deflate.h) that images do not reach, and a numpy restatement of the
encoder's contract to build them with: the token parse of a segment, unlimited Huffman depths by a heap, the encoder's own length-limited lengths and
the run-length coding of the code-length sequence (RFC 1951 3.2.7).  No GPU, no project import: test_deflate_inputs_cpu.py asserts what each builder
promises, test_deflate_adversarial.py feeds them to the device."""
import heapq

import numpy as np

SEG = 16384           # kZipSeg: bytes per segment, one deflate block each
SPAN = 64             # kZipSpan: bytes one thread parses
LEN_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
RUN_Q, RUN_R, RUN_OFF = (0, 1, 2), (0, 1, 2, 3, 4, 257), (0, 1, 62, 63)


def segments(x):
    x = np.asarray(x, np.uint8)
    return [x[o:o + SEG] for o in range(0, len(x), SEG)]


def runs(x):
    """maximal runs of equal bytes -> (start, length, value) arrays"""
    x = np.asarray(x, np.uint8)
    start = np.flatnonzero(np.concatenate([[True], x[1:] != x[:-1]]))
    return start, np.diff(np.concatenate([start, [len(x)]])), x[start]


def length_symbol(n):
    """match length 3..258 -> its symbol 257..285 (258 has a code of its own)"""
    return 257 + np.searchsorted(LEN_BASE, n, side="right") - 1


def tokens(segment):
    """hist[286] of one segment's tokens.  Per run: one literal, rest // 258 matches of 258, then a match of rest % 258 when that is at least 3,
    otherwise that many literals; the end-of-block symbol once."""
    assert 0 < len(segment) <= SEG
    hist = np.zeros(286, np.int64)
    _, n, v = runs(segment)
    q, r = np.divmod(n - 1, 258)
    np.add.at(hist, v, 1 + np.where(r < 3, r, 0))
    hist[285] += q.sum()
    np.add.at(hist, length_symbol(r[r >= 3]), 1)
    hist[256] = 1
    return hist


def token_list(segment):
    """the same parse in stream order: a literal is its byte value, a match is (length, 1)"""
    assert 0 < len(segment) <= SEG
    out = []
    for n, v in zip(*runs(segment)[1:]):
        q, r = divmod(int(n) - 1, 258)
        out += [int(v)] + [(258, 1)] * q + ([(r, 1)] if r >= 3 else [int(v)] * r)
    return out


def huffman_depths(hist):
    """unlimited Huffman code depths of the used symbols (0 for an unused one), by a plain heap"""
    hist = np.asarray(hist)
    depth = np.zeros(len(hist), np.int64)
    heap = [(int(f), s, [s]) for s, f in enumerate(hist) if f]
    if len(heap) == 1:
        depth[heap[0][1]] = 1
    heapq.heapify(heap)
    tie = len(hist)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        depth[a + b] += 1
        heapq.heappush(heap, (fa + fb, tie, a + b))
        tie += 1
    return depth


def limited_lengths(hist, maxlen):
    """The encoder's code lengths, step for step as zip_huff_lengths computes them: used symbols sorted by (count, symbol), the in-place
    minimum-redundancy algorithm of Moffat & Katajainen, depths beyond maxlen clamped, then codes moved down the length counts until the Kraft
    sum is 1; the rarest symbols get the longest codes.  -> (lengths, deepest unlimited depth)"""
    hist = np.asarray(hist)
    lens = np.zeros(len(hist), np.int64)
    sym = sorted((s for s in range(len(hist)) if hist[s]), key=lambda s: (int(hist[s]), s))
    nz = len(sym)
    if nz == 1:
        lens[sym[0]] = 1
        lens[1 if sym[0] == 0 else 0] = 1
        return lens, 1
    if nz == 0:
        return lens, 0
    A = [int(hist[s]) for s in sym]
    A[0] += A[1]
    root, leaf = 0, 2
    for nxt in range(1, nz - 1):
        if leaf >= nz or A[root] < A[leaf]:
            A[nxt] = A[root]; A[root] = nxt; root += 1
        else:
            A[nxt] = A[leaf]; leaf += 1
        if leaf >= nz or (root < nxt and A[root] < A[leaf]):
            A[nxt] += A[root]; A[root] = nxt; root += 1
        else:
            A[nxt] += A[leaf]; leaf += 1
    A[nz - 2] = 0
    for nxt in range(nz - 3, -1, -1):
        A[nxt] = A[A[nxt]] + 1
    avbl, used, dpth, root, nxt = 1, 0, 0, nz - 2, nz - 1
    while avbl > 0:
        while root >= 0 and A[root] == dpth:
            used += 1; root -= 1
        while avbl > used:
            A[nxt] = dpth; nxt -= 1; avbl -= 1
        avbl, dpth, used = 2 * used, dpth + 1, 0
    deepest = max(A)
    blc = [0] * (max(deepest, maxlen) + 1)
    for d in A:
        blc[min(d, maxlen)] += 1
    total = sum(blc[i] << (maxlen - i) for i in range(1, maxlen + 1))
    while total > (1 << maxlen):
        blc[maxlen] -= 1
        for i in range(maxlen - 1, 0, -1):
            if blc[i]:
                blc[i] -= 1; blc[i + 1] += 2
                break
        total -= 1
    j = 0
    for i in range(maxlen, 0, -1):
        for _ in range(blc[i]):
            lens[sym[j]] = i; j += 1
    return lens, deepest


def code_length_sequence(lengths):
    """literal/length code lengths (286) -> the code-length symbols the header sends, as (symbol, extra) pairs: the HLIT lengths followed by the
    single distance length 1, zeros coded with 18 for runs of 11 to 138 then 17 for runs of 3 to 10, a non-zero length once then 16 for runs of 3 to 6"""
    hlit = 286
    while hlit > 257 and lengths[hlit - 1] == 0:
        hlit -= 1
    seq = [int(v) for v in lengths[:hlit]] + [1]
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138); out.append((18, r - 11)); run -= r
            if run >= 3:
                out.append((17, run - 3)); run = 0
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                r = min(run, 6); out.append((16, r - 3)); run -= r
        out += [(v, 0)] * run
    return out


def code_length_histogram(lengths):
    hist = np.zeros(19, np.int64)
    for s, _ in code_length_sequence(lengths):
        hist[s] += 1
    return hist


def _no_equal_neighbours(values, counts):
    """counts[i] copies of values[i], no two equal bytes next to each other: the even positions are filled first, then the odd ones, in order of
    falling count (every count is below half the total)"""
    order = np.argsort(-np.asarray(counts), kind="stable")
    seq = np.repeat(np.asarray(values, np.uint8)[order], np.asarray(counts)[order])
    assert 2 * max(counts) < len(seq)
    out = np.empty(len(seq), np.uint8)
    half = (len(seq) + 1) // 2
    out[0::2] = seq[:half]
    out[1::2] = seq[half:]
    return out


def deep_literal_code():
    """18 byte values with the counts 1, 2, 3, 5, 8, ..., 4181 (10 944 bytes, no runs).  With the end-of-block symbol the weights are 1, 1, 2, 3, 5, ...:
    at every step the two smallest are the merged node and the next leaf, so the unlimited code is a chain of depth 18 whatever the tie-break, and
    the 15-bit limiter has to run."""
    counts = [1, 2]
    while len(counts) < 18:
        counts.append(counts[-1] + counts[-2])
    return _no_equal_neighbours([7 + 13 * i for i in range(18)], counts)


CL_SEED, CL_DRAW = 0, 2         # CL_DRAW: the first draw of search_deep_code_length_code(CL_SEED) that qualifies


def _cl_draw(seed, draw):
    """One candidate for deep_code_length_code: a number of byte values for each code length 2..11 that fills the Kraft sum, counts near
    16000 * 2^-k, byte values permuted so that equal lengths rarely neighbour in the code-length sequence.  None when it does not fit a segment."""
    rng = np.random.default_rng([seed, draw])
    avail, per_len = 4, []
    for k in range(2, 12):
        n = avail if k == 11 else min(avail - 1, int(rng.integers(0, max(1, int(avail * 0.6)) + 1)))
        per_len.append(n)
        avail = 2 * (avail - n)
    per_len[-1] -= 1                                                   # the end-of-block symbol takes one of the longest codes
    if not 0 < sum(per_len) <= 256:
        return None
    counts = [max(1, int(round(16000.0 * 2.0 ** -k * rng.uniform(0.85, 1.15)))) for k, n in zip(range(2, 12), per_len) for _ in range(n)]
    if sum(counts) > SEG or 2 * max(counts) >= sum(counts):
        return None
    return _no_equal_neighbours(rng.permutation(256)[:len(counts)], counts)


def code_length_code_depths(segment):
    """-> (heap depth, the encoder's own unlimited depth) of the code-length code of one segment's limited literal/length code"""
    clh = code_length_histogram(limited_lengths(tokens(segment), 15)[0])
    return int(huffman_depths(clh).max()), int(limited_lengths(clh, 7)[1])


def search_deep_code_length_code(seed=CL_SEED, draws=3000):
    """the first draw whose code-length code is deeper than 7 bits both by the heap and by the encoder's own algorithm (ties may differ)"""
    for draw in range(draws):
        x = _cl_draw(seed, draw)
        if x is not None and min(code_length_code_depths(x)) >= 8:
            return draw
    raise RuntimeError("no draw reaches depth 8")


def deep_code_length_code():
    """One segment, no runs, whose limited literal/length lengths give a code-length histogram of unlimited depth >= 8: the 7-bit limiter has to run."""
    return _cl_draw(CL_SEED, CL_DRAW)


class _Filler:
    """single bytes of changing value below 200 (run values are 200 and above): no filler byte equals a neighbour"""
    def __init__(self):
        self.k = 0

    def __call__(self, n):
        out = (self.k + np.arange(n)) % 200
        self.k = (self.k + n) % 200
        return out.astype(np.uint8)


def run_table():
    """Three segments.  Runs of 1 + 258 q + r bytes for q in RUN_Q and r in RUN_R, each starting at the offsets RUN_OFF modulo SPAN and none of them
    across a segment edge; neighbouring runs differ in value, single filler bytes set the offsets.  Then the edges: one run over bytes 16 380..16 390
    (the encoder has to split it, host zlib sees it whole) and one run that ends exactly at the edge 32 768, followed by a last short segment."""
    fill, parts, pos, k = _Filler(), [], 0, 0
    edge = [False]

    def put(a):
        nonlocal pos
        parts.append(np.asarray(a, np.uint8)); pos += len(a)

    def run(n):
        nonlocal k
        put(np.full(n, 200 + k % 56, np.uint8)); k += 1

    def cross():                                                       # filler up to 16 380, then the run over the edge
        put(fill(SEG - 4 - pos)); run(11); edge[0] = True

    for q in RUN_Q:
        for r in RUN_R:
            for off in RUN_OFF:
                n = 1 + 258 * q + r
                pad = (off - pos) % SPAN
                if not edge[0] and pos + pad + n > SEG - 4:
                    cross()
                    pad = (off - pos) % SPAN
                put(fill(pad)); run(n)
    assert edge[0] and pos < 2 * SEG - 600
    put(fill(2 * SEG - 300 - pos)); run(300)                           # ends exactly at 32 768
    put(fill(1)); run(300); put(fill(3))
    return np.concatenate(parts)


def one_byte_segment(v):
    return np.full(SEG, v, np.uint8)


def every_symbol():
    """every byte value at least once and one run for each of the 29 length codes: all 286 literal/length symbols are used (HLIT = 286)"""
    parts = [np.full(1 + int(n), i, np.uint8) for i, n in enumerate(LEN_BASE)]
    return np.concatenate(parts + [np.arange(256, dtype=np.uint8)])


def high_bytes(n, seed):
    """uniform in 0xF0..0xFF: compresses a little (4 bits a byte) and is the worst case for the Adler-32 sums"""
    return np.random.default_rng([1, seed]).integers(0xF0, 0x100, n, dtype=np.uint8)


def noise(n, seed):
    """uniform bytes: at segment size they end up as stored blocks"""
    return np.random.default_rng([2, seed]).integers(0, 256, n, dtype=np.uint8)
