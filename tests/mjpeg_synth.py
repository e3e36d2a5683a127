"""A baseline JPEG stream writer for the MJPEG decoder's tests, written from the standard (ITU-T T.81): SOI, JFIF APP0, COM, DQT,
SOF0, DHT, DRI, SOS, Huffman-coded interleaved scan with byte stuffing, 1-bit padding and RSTn cycling, EOI.  It exists to
reach what no encoder writes: every run/size symbol, ZRL chains, blocks that end without EOB, code lengths up to 16, table ids 2
and 3, fill bytes in front of RSTn, restart intervals of any length.  The streams are decoded by Pillow / libjpeg-turbo and by
mjpeg_ref.py in test_mjpeg_synth_cpu.py (which pins them to each other) and by the device against mjpeg_ref.py.

THE DOMAIN.  Every stream held against a reference satisfies  extent(stream) <= DOMAIN = 16384  in both figures: the largest
|dequantised coefficient| and the largest |value of the IDCT workspace| (the output of the column pass, mjpeg_ref._pass(cols,
11, 1024)).  Inside it

  * the decoder's 16-bit saturation (mjpeg_sat16) never acts: 16384 < 32767;
  * Pillow / libjpeg-turbo and rule J2 agree.  They part once the workspace nears the 16-bit range (measured with Pillow 12.2:
    streams whose workspace stayed within +-25455 agreed exactly, every stream that reached +-28718 differed in a few pixels);
  * 32-bit IDCT arithmetic cannot wrap.  One ISLOW pass is linear in its eight inputs up to the final rounding, so every
    intermediate is a linear form  sum a_k x_k  and |form| <= (sum |a_k|) X  for inputs |x_k| <= X.  islow_gain() replays the
    butterfly on such forms and returns the largest sum |a_k| over ALL intermediates and outputs: 61214.  The column pass
    sees coefficients, the row pass sees the workspace, both <= 16384, so every value stays below 61214 * 16384 + 131072 =
    1 003 061 248 < 2^31 - 1: a factor 2.1 to spare.  (Bounding term by term instead gives about 1.7e5 X, which would NOT
    suffice; the difference is terms like z3 * -16069 + z5, which as one form is -6436 (x7 + x3) + 9633 (x5 + x1): 32138,
    not 70670.)  test_mjpeg_synth_cpu.py recomputes the figure and asserts the inequality.

Generators CONSTRUCT streams inside the domain: into_domain() scales the AC magnitudes of a block whose workspace would leave
it; nothing is filtered by rejection, so no case is silently left out.  Tests assert the condition for every stream they use.

Coefficient arrays are per component [blocks_y, blocks_x, 64], quantised, in zigzag order, on the padded MCU grid of the
interleaved scan (one component: ceil(H/8) x ceil(W/8))."""
import collections

import numpy as np

import mjpeg_ref as ref

DOMAIN = 16384
SAMPLINGS = {"gray": (1, 1, 1), "1x1": (3, 1, 1), "2x1": (3, 2, 1), "2x2": (3, 2, 2)}       # components, luma h, luma v
AC_SYMBOLS = [r << 4 | s for r in range(16) for s in range(1, 11)] + [0x00, 0xF0]          # 160 run/size, EOB, ZRL
DC_SYMBOLS = list(range(12))


# ---- Huffman tables -----------------------------------------------------------------------------------------------------------
def huffman_table(symbols, profile, seed):
    """A legal table (bits[16], vals) for `symbols`: code counts per length follow `profile`, which symbol gets which length is
    seeded.  Legal as libjpeg demands: the counts satisfy Kraft's inequality with the all-ones code of every length left free.

    profile: "flat"      every code as short as the count allows (all within the 8-bit look-up for 162 symbols)
             "boundary"  one short code, a third of the symbols at exactly 8 bits, a third at exactly 9, the rest deeper
             "deep"      one code at each of the lengths 1-8, then as the room allows: the deepest level holds most symbols
             "chain"     one code at every length from 1 on (all sixteen lengths for exactly 16 symbols)
             "random"    0-3 codes per length, seeded
             or a list of 16 wanted counts.
    Wanted counts are cut to what leaves room for the remaining symbols at 16 bits; what is left over goes to 16 bits."""
    rng = np.random.default_rng(seed)
    vals = [int(v) for v in symbols]
    rng.shuffle(vals)
    n = len(vals)
    if profile == "flat":
        want = [0] * 16
        want[max(1, int(n).bit_length()) - 1] = n          # 2^length >= n + 1
    elif profile == "boundary":
        want = [0] * 16
        want[2], want[7], want[8] = 1, max(1, n // 3), max(1, n // 3)
    elif profile == "deep":
        want = [1] * 8 + [0] * 8
    elif profile == "chain":
        want = [1] * 16
    elif profile == "random":
        want = [int(v) for v in rng.integers(0, 4, 16)]
    else:
        want = [int(v) for v in profile]
    bits, left, space = [0] * 16, n, 65535            # space in units of 2^-16; the 65536th is the all-ones code
    for length in range(1, 16):
        cost = 1 << (16 - length)
        take = max(0, min(want[length - 1], left, (space - left) // (cost - 1)))
        bits[length - 1] = take
        left -= take
        space -= take * cost
    bits[15] = left
    assert left <= space, "no room for %d symbols" % n
    return bits, vals


def check_table(bits, vals):
    """what jpeg_make_d_derived_tbl demands: after the codes of each length the next code still fits that length"""
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        assert code < (1 << length), "codes of length %d do not fit" % length
        code <<= 1
    assert sum(bits) == len(vals) <= 256 and len(set(vals)) == len(vals)


def lengths_of(table):
    bits, vals = table
    out, k = {}, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = length
            k += 1
    return out


def _encoder(table):
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def tables(profile, seed, ids=((0, 0), (0, 1), (1, 0), (1, 1)), symbols=None):
    """{(class, id): table} of generated tables; symbols: {class: symbol list} (all twelve DC / all 162 AC by default)"""
    symbols = symbols or {}
    return {(cls, i): huffman_table(symbols.get(cls, AC_SYMBOLS if cls else DC_SYMBOLS), profile, seed * 16 + cls * 4 + i)
            for cls, i in ids}


# ---- the writer ---------------------------------------------------------------------------------------------------------------
class _BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, length):
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.n -= 8
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)                      # byte stuffing
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)      # padded with 1-bits


def _size(v):
    return int(abs(v)).bit_length()


def _amplitude(v, s):
    return v if v >= 0 else v + (1 << s) - 1


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def write(W, H, sampling, blocks, quant, huff=None, comp_q=None, comp_h=None, ri=0, fill=0, emit_dht=True, packed=False,
          huff_first=None, comment=b"", log=None):
    """-> the stream (bytes).

    sampling   "gray", "1x1", "2x1" or "2x2" (the luma factors; chroma is 1 x 1)
    blocks     per component [blocks_y, blocks_x, 64] quantised coefficients, zigzag order
    quant      {id 0-3: 64 values 1-255, zigzag order};  comp_q: the id of each component (default 0, 1, 1)
    huff       {(class, id 0-3): (bits, vals)}, the tables the scan is coded with (default: the standard's, ids 0 and 1);
               comp_h: per component (DC id, AC id) (default (0, 0), (1, 1), (1, 1))
    ri         the DRI value, 0 for no DRI segment;  fill: 0xFF fill bytes in front of every RSTn
    emit_dht   False: no DHT at all (the decoder's built-in tables; `huff` must then be the standard's under ids 0 / 1)
    packed     True: all quantisers in one DQT segment and all Huffman tables in one DHT; False: one segment each
    huff_first tables written in DHT segments of their own BEFORE those of `huff`: a later definition of an id replaces them
    comment    a COM segment's payload (also a way to choose the stream's length)
    log        a collections.Counter: counts ("dc", category) and ("ac", run/size symbol) as they are coded"""
    nc, hs, vs = SAMPLINGS[sampling]
    huff = ref.std_tables() if huff is None else huff
    comp_q = comp_q or (0, 1, 1)[:nc]
    comp_h = comp_h or ((0, 0), (1, 1), (1, 1))[:nc]
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    assert len(blocks) == nc
    for c in range(nc):
        h, v = (hs, vs) if c == 0 else (1, 1)
        assert blocks[c].shape == (mcuy * v, mcux * h, 64), (c, blocks[c].shape, (mcuy * v, mcux * h, 64))
    o = bytearray(b"\xff\xd8") + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if comment:
        o += _seg(0xFE, comment)
    dqt = [bytes([i]) + bytes(int(x) for x in quant[i]) for i in sorted(quant)]
    assert all(len(t) == 65 and 0 not in t[1:] for t in dqt)
    for t in ([b"".join(dqt)] if packed else dqt):
        o += _seg(0xDB, t)
    sof = b"\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        sof += bytes([c + 1, ((hs << 4) | vs) if c == 0 else 0x11, comp_q[c]])
    o += _seg(0xC0, sof)
    if emit_dht:
        for (cls, i), (bits, vals) in (huff_first or {}).items():
            o += _seg(0xC4, bytes([cls << 4 | i]) + bytes(bits) + bytes(vals))
        dht = [bytes([cls << 4 | i]) + bytes(bits) + bytes(vals) for (cls, i), (bits, vals) in sorted(huff.items())]
        for t in ([b"".join(dht)] if packed else dht):
            o += _seg(0xC4, t)
    if ri:
        o += _seg(0xDD, ri.to_bytes(2, "big"))
    sos = bytes([nc])
    for c in range(nc):
        sos += bytes([c + 1, comp_h[c][0] << 4 | comp_h[c][1]])
    o += _seg(0xDA, sos + b"\x00\x3f\x00")
    enc = [(_encoder(huff[(0, comp_h[c][0])]), _encoder(huff[(1, comp_h[c][1])])) for c in range(nc)]
    total = mcux * mcuy
    per = ri if ri else total
    rst = 0
    for first in range(0, total, per):
        bw, pred = _BitWriter(), [0] * nc
        for mcu in range(first, min(total, first + per)):
            my, mx = divmod(mcu, mcux)
            for c in range(nc):
                h, v = (hs, vs) if c == 0 else (1, 1)
                dc, ac = enc[c]
                for j in range(v):
                    for i in range(h):
                        blk = [int(x) for x in blocks[c][my * v + j, mx * h + i]]
                        diff, pred[c] = blk[0] - pred[c], blk[0]
                        s = _size(diff)
                        assert s <= 11, "DC difference %d" % diff
                        bw.put(*dc[s])
                        if s:
                            bw.put(_amplitude(diff, s), s)
                        if log is not None:
                            log[("dc", s)] += 1
                        run = 0
                        for k in range(1, 64):
                            a = blk[k]
                            if a == 0:
                                run += 1
                                continue
                            while run > 15:
                                bw.put(*ac[0xF0])                  # ZRL
                                run -= 16
                                if log is not None:
                                    log[("ac", 0xF0)] += 1
                            s = _size(a)
                            assert s <= 10, "AC value %d" % a
                            bw.put(*ac[run << 4 | s])
                            bw.put(_amplitude(a, s), s)
                            if log is not None:
                                log[("ac", run << 4 | s)] += 1
                            run = 0
                        if run:                                    # EOB, unless coefficient 63 is there
                            bw.put(*ac[0x00])
                            if log is not None:
                                log[("ac", 0x00)] += 1
        bw.flush()
        o += bw.out
        if first + per < total:
            o += b"\xff" * fill + bytes([0xFF, 0xD0 + rst])
            rst = (rst + 1) & 7
    return bytes(o + b"\xff\xd9")


# ---- the domain ---------------------------------------------------------------------------------------------------------------
def _natural(blocks):
    out = np.zeros(blocks.shape, np.int64)
    out[..., ref.ZIGZAG] = blocks
    return out


def _workspace(natural):
    """the column pass of J2 on [..., 64] natural-order dequantised coefficients"""
    c = natural.reshape(natural.shape[:-1] + (8, 8)).astype(np.int64)
    return ref._pass(np.swapaxes(c, -1, -2), 11, 1024)


def extent(stream, default_tables=None):
    """(largest |dequantised coefficient|, largest |workspace value|) that mjpeg_ref computes for the stream"""
    coef = ref.coefficients(ref.parse(stream, default_tables))
    return (max(int(np.abs(c).max()) for c in coef), max(int(np.abs(_workspace(c)).max()) for c in coef))


def in_domain(stream, default_tables=None):
    return max(extent(stream, default_tables)) <= DOMAIN


def into_domain(blocks, q, limit=DOMAIN * 3 // 4):
    """Scales (towards zero) the AC values of every block of one component whose dequantised coefficients or workspace would
    exceed `limit`; the DC value too where it alone is too large.  q: the component's quantiser, zigzag.  -> a new array."""
    b = np.array(blocks, np.int64)
    q = np.asarray(q, np.int64)
    for _ in range(64):
        nat = _natural(b * q)
        worst = np.maximum(np.abs(nat).max(-1), np.abs(_workspace(nat)).reshape(b.shape[:-1] + (64,)).max(-1))
        bad = worst > limit
        if not bad.any():
            return b
        f = (limit / worst[bad])[:, None] * 0.9
        ac = b[bad]
        dc_alone = np.abs(ac[:, 0] * q[0]) * 4 + 4 > limit * 0.9
        ac[:, 1:] = np.trunc(ac[:, 1:] * f)
        ac[dc_alone, 0] = np.trunc(ac[dc_alone, 0] * f[dc_alone, 0])
        b[bad] = ac
    raise AssertionError("into_domain did not converge")


class _Form:
    """a linear form in x0..x7 with integer coefficients"""
    def __init__(self, a):
        self.a = np.asarray(a, np.int64)

    def __add__(self, o):
        return _Form(self.a + o.a)

    def __sub__(self, o):
        return _Form(self.a - o.a)

    def __mul__(self, k):
        return _Form(self.a * k)


def islow_gain():
    """The largest sum of |coefficients| over every intermediate and output of one ISLOW pass (jidctint's butterfly, as in
    mjpeg_ref._pass and islow_pass of k_mjpeg.hip), each taken as a linear form in the pass's eight inputs."""
    x = [_Form(np.eye(8, dtype=np.int64)[i]) for i in range(8)]
    seen = []

    def t(f):
        seen.append(int(np.abs(f.a).sum()))
        return f

    z2, z3 = x[2], x[6]
    z1 = t(t(z2 + z3) * 4433)
    tmp2 = t(z1 - t(z3 * 15137))
    tmp3 = t(z1 + t(z2 * 6270))
    tmp0 = t(t(x[0] + x[4]) * 8192)
    tmp1 = t(t(x[0] - x[4]) * 8192)
    t10, t13, t11, t12 = t(tmp0 + tmp3), t(tmp0 - tmp3), t(tmp1 + tmp2), t(tmp1 - tmp2)
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = t(tmp0 + tmp3), t(tmp1 + tmp2), t(tmp0 + tmp2), t(tmp1 + tmp3)
    z5 = t(t(z3 + z4) * 9633)
    tmp0, tmp1, tmp2, tmp3 = t(tmp0 * 2446), t(tmp1 * 16819), t(tmp2 * 25172), t(tmp3 * 12299)
    z1, z2 = t(z1 * -7373), t(z2 * -20995)
    z3, z4 = t(t(z3 * -16069) + z5), t(t(z4 * -3196) + z5)
    tmp0, tmp1, tmp2, tmp3 = t(t(tmp0 + z1) + z3), t(t(tmp1 + z2) + z4), t(t(tmp2 + z2) + z3), t(t(tmp3 + z1) + z4)
    for even, odd in ((t10, tmp3), (t11, tmp2), (t12, tmp1), (t13, tmp0)):
        t(even + odd)
        t(even - odd)
    return max(seen)


# ---- an encoder's forward path ------------------------------------------------------------------------------------------------
def _dct_matrix():
    k, n = np.mgrid[0:8, 0:8]
    m = np.cos((2 * n + 1) * k * np.pi / 16) * 0.5
    m[0] /= np.sqrt(2)
    return m


_DCT = _dct_matrix()


def blocks_from_planes(planes, quantisers):
    """planes: per component a uint8 / float array on the padded grid (multiples of 8); quantisers: per component 64 values,
    zigzag -> per component [by, bx, 64] quantised, zigzag: level shift, float DCT, division, rounding.  DC is kept within
    [-1024, 1023] and AC within +-1023 of the DEQUANTISED scale's legal codes (sizes 11 and 10)."""
    out = []
    for p, q in zip(planes, quantisers):
        p = np.asarray(p, np.float64) - 128.0
        by, bx = p.shape[0] // 8, p.shape[1] // 8
        b = p.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3)
        f = np.einsum("ij,yxjk,lk->yxil", _DCT, b, _DCT).reshape(by, bx, 64)
        qn = np.zeros(64)
        qn[ref.ZIGZAG] = np.asarray(q, np.float64)
        z = np.rint(f / qn)[..., ref.ZIGZAG].astype(np.int64)
        z[..., 0] = np.clip(z[..., 0], -1024, 1023)
        z[..., 1:] = np.clip(z[..., 1:], -1023, 1023)
        out.append(z)
    return out


def blocks_from_image(img, quantisers, sampling):
    """What an encoder does with img (H x W x 3 RGB uint8, or H x W for "gray"): JFIF's YCbCr, the edge replicated up to the MCU
    grid, chroma box-averaged over the luma factors, then blocks_from_planes."""
    nc, hs, vs = SAMPLINGS[sampling]
    img = np.asarray(img, np.float64)
    H, W = img.shape[:2]
    Hp, Wp = -(-H // (8 * vs)) * 8 * vs, -(-W // (8 * hs)) * 8 * hs
    img = np.pad(img, ((0, Hp - H), (0, Wp - W)) + ((0, 0),) * (img.ndim - 2), mode="edge")
    if nc == 1:
        return blocks_from_planes([img if img.ndim == 2 else img[..., 1]], quantisers)
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb = -0.168735892 * r - 0.331264108 * g + 0.5 * b + 128
    cr = 0.5 * r - 0.418687589 * g - 0.081312411 * b + 128
    box = lambda p: p.reshape(Hp // vs, vs, Wp // hs, hs).mean((1, 3))      # noqa: E731
    return blocks_from_planes([y, box(cb), box(cr)], quantisers)


def grid(W, H, sampling):
    """per component (blocks_y, blocks_x) of the padded MCU grid"""
    nc, hs, vs = SAMPLINGS[sampling]
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    return [(mcuy * vs, mcux * hs)] + [(mcuy, mcux)] * (nc - 1)


def launch_shape(stream, default_tables=None):
    """(segments, blocks per frame, first block of each component) as launch_mjpeg sees the frame"""
    f = ref.parse(stream, default_tables)
    g = grid(f.W, f.H, {(1, 1, 1): "gray", (3, 1, 1): "1x1", (3, 2, 1): "2x1", (3, 2, 2): "2x2"}[(f.ncomp, f.hs, f.vs)])
    first = [0]
    for by, bx in g:
        first.append(first[-1] + by * bx)
    return len(f.segments), first[-1], first[:-1]


# ---- the stream classes of the tests (a-e) --------------------------------------------------------------------------------------
# Each class is a list of (label, stream).  test_mjpeg_synth_cpu.py holds every one against Pillow, the host build and the
# sanitized host build; test_gpu_mjpeg_synth.py gives the same streams to the device.
SEEDS = (1, 2, 3)
PROFILES = ("boundary", "deep", "random")


def _texture(W, H, seed):
    import sys
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    import make_mjpeg_golden
    return make_mjpeg_golden.texture(W, H, seed)


def _value(rng, s):
    """a value of size category s (magnitude 2^(s-1) .. 2^s - 1), random sign"""
    v = int(rng.integers(1 << (s - 1), 1 << s))
    return v if rng.integers(0, 2) else -v


def coverage_blocks(seed):
    """Blocks (zigzag, for quantiser 1) that between them code all 160 run/size symbols, ZRL, EOB and DC categories 0-11.  At most
    two values of size 8-10 share a block, so the workspace stays far inside the domain."""
    rng = np.random.default_rng(seed)
    todo = [(r, s) for r in range(16) for s in range(1, 11)]
    order = rng.permutation(len(todo))
    out, blk, k, large = [], np.zeros(64, np.int64), 1, 0
    for idx in order:
        r, s = todo[idx]
        if k + r > 63 or (s >= 8 and large == 2):
            out.append(blk)
            blk, k, large = np.zeros(64, np.int64), 1, 0
        blk[k + r] = _value(rng, s)
        k += r + 1
        large += s >= 8
    out.append(blk)
    far = np.zeros(64, np.int64)
    far[40] = _value(rng, 3)                    # 39 zeros: two ZRLs and a run of 7
    out.append(far)
    dcs = [0, 1, -2, 4, -8, 16, -32, 64, -128, 256, -512, 1023]       # differences of categories 0 .. 11 after a leading 0
    assert len(out) >= len(dcs) + 1
    out[0][0] = 0
    for i, d in enumerate(dcs):
        out[i + 1][0] = d
    return out


def arrange(blocks, sampling):
    """One MCU row of len(blocks) MCUs whose every component walks through `blocks` (the luma blocks of MCU m in coding order
    take blocks[m * h * v + ...], Cb starts one further, Cr two): -> (W, H, per-component arrays)"""
    nc, hs, vs = SAMPLINGS[sampling]
    n = len(blocks)
    comps = [np.zeros((vs, n * hs, 64), np.int64)] + [np.zeros((1, n, 64), np.int64) for _ in range(nc - 1)]
    for m in range(n):
        for j in range(vs):
            for i in range(hs):
                comps[0][j, m * hs + i] = blocks[(m * hs * vs + j * hs + i) % n]
        for c in range(1, nc):
            comps[c][0, m] = blocks[(m + c) % n]
    return n * 8 * hs, 8 * vs, comps


def unit_quant():
    return {0: np.ones(64, np.int64), 1: np.ones(64, np.int64)}


def class_a(seed, logs=None):
    """symbol coverage: gray and 2x1, the standard tables and three generated length profiles"""
    out = []
    blocks = coverage_blocks(seed)
    for sampling in ("gray", "2x1"):
        W, H, comps = arrange(blocks, sampling)
        for prof in ("std",) + PROFILES:
            log = collections.Counter()
            huff = None if prof == "std" else tables(prof, seed)
            out.append(("a/%s/%s/seed%d" % (sampling, prof, seed), write(W, H, sampling, comps, unit_quant(), huff, ri=7, log=log)))
            if logs is not None:
                logs.append(log)
    return out


def shape_blocks(seed):
    rng = np.random.default_rng(100 + seed)
    z = lambda: np.zeros(64, np.int64)            # noqa: E731
    b = [z() for _ in range(10)]
    b[0][[0, 5, 63]] = [17, _value(rng, 4), _value(rng, 2)]          # coefficient 63 present: no EOB
    b[1][63] = _value(rng, 3)                                         # only coefficient 63
    b[2][[0, 52]] = [-9, _value(rng, 5)]                              # 51 zeros: three ZRLs, then run 3
    b[3][0] = 40
    b[3][1:] = [_value(rng, int(rng.integers(1, 4))) for _ in range(63)]      # all 63 AC present
    b[4][0] = -77                                                     # DC only
    b[5][0], b[6][0], b[7][0], b[8][0] = -1024, 1023, -1024, 1023     # DC differences of +-2047, inside an MCU's luma blocks too
    b[9][49] = _value(rng, 6)                                         # 48 zeros: exactly three ZRLs, then run 0
    return b


def class_b(seed):
    """block shapes, in every component of gray, 2x1 and 2x2 frames"""
    out = []
    blocks = shape_blocks(seed)
    for sampling in ("gray", "2x1", "2x2"):
        W, H, comps = arrange(blocks, sampling)
        for prof in ("std", PROFILES[seed % 3], "chain"):
            huff = None if prof == "std" else tables(prof, 40 + seed)
            out.append(("b/%s/%s/seed%d" % (sampling, prof, seed), write(W, H, sampling, comps, unit_quant(), huff, ri=4)))
    return out


def _random_quant(rng, lo=1, hi=256):
    return rng.integers(lo, hi, 64).astype(np.int64)


def _encoded(img, sampling, quants):
    """blocks_from_image with the component quantisers `quants`, brought into the domain"""
    nc = SAMPLINGS[sampling][0]
    src = img if nc == 3 else img[..., 1]
    return [into_domain(b, q) for b, q in zip(blocks_from_image(src, quants[:nc], sampling), quants[:nc])]


def class_c(seed):
    """table plumbing"""
    rng = np.random.default_rng(200 + seed)
    out = []
    W, H = 24, 16
    img = _texture(W, H, 50 + seed)
    q = [_random_quant(rng, 1, 40) for _ in range(3)]

    def add(label, sampling, *args, **kw):
        out.append(("c/%s/seed%d" % (label, seed), write(W, H, sampling, *args, **kw)))

    col = _encoded(img, "2x1", q)
    t = tables("random", 60 + seed, ids=[(c, i) for c in (0, 1) for i in range(4)])
    # ids 2 and 3 only
    add("ids23", "2x1", _encoded(img, "2x1", [q[0], q[1], q[1]]), {3: q[0], 2: q[1]}, {k: t[k] for k in ((0, 3), (1, 2), (0, 2), (1, 3))},
        comp_q=(3, 2, 2), comp_h=((3, 2), (2, 3), (2, 3)))
    # Cb and Cr differ in quantiser and in both Huffman tables
    add("cbcr_differ", "2x1", col, {0: q[0], 1: q[1], 2: q[2]}, {k: t[k] for k in ((0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2))},
        comp_q=(0, 1, 2), comp_h=((0, 0), (1, 1), (2, 2)))
    # one quantiser, one DC and one AC table for all three
    add("shared", "2x1", _encoded(img, "2x1", [q[0]] * 3), {0: q[0]}, {k: t[k] for k in ((0, 0), (1, 0))}, comp_q=(0, 0, 0),
        comp_h=((0, 0),) * 3)
    add("gray_id3", "gray", _encoded(img, "gray", [q[2]]), {3: q[2]}, {k: t[k] for k in ((0, 3), (1, 3))}, comp_q=(3,), comp_h=((3, 3),))
    std = _encoded(img, "2x1", [q[0], q[1], q[1]])
    add("no_dht", "2x1", std, {0: q[0], 1: q[1]}, None, emit_dht=False)
    add("no_dht_gray", "gray", _encoded(img, "gray", [q[0]]), {0: q[0]}, None, emit_dht=False, comp_q=(0,))
    four = {k: t[k] for k in ((0, 0), (1, 0), (0, 1), (1, 1))}
    add("packed", "2x1", std, {0: q[0], 1: q[1]}, four, packed=True)
    add("separate", "2x1", std, {0: q[0], 1: q[1]}, four, packed=False)
    # every id is defined twice before SOS: the later definition is the one the scan is coded with
    decoy = tables("deep", 90 + seed)
    assert all(decoy[k] != four[k] for k in four)
    add("redefined", "2x1", std, {0: q[0], 1: q[1]}, four, huff_first=decoy)
    return out


def class_d(seed):
    """restart structure"""
    rng = np.random.default_rng(300 + seed)
    out = []
    W, H = 72, 40
    for sampling in SAMPLINGS:
        nc, hs, vs = SAMPLINGS[sampling]
        mcux, total = -(-W // (8 * hs)), -(-W // (8 * hs)) * -(-H // (8 * vs))
        q = [_random_quant(rng, 1, 12) for _ in range(2)]
        comps = []
        for c, (by, bx) in enumerate(grid(W, H, sampling)):
            b = np.zeros((by, bx, 64), np.int64)
            b[..., 0] = rng.integers(-60, 60, (by, bx))
            for _ in range(4):
                k = rng.integers(1, 64, (by, bx))
                np.put_along_axis(b, k[..., None], rng.integers(-30, 31, (by, bx, 1)), -1)
            comps.append(into_domain(b, q[min(c, 1)], limit=DOMAIN // 2))
        quant = {0: q[0], 1: q[1]}
        huff = tables(PROFILES[seed % 3], 70 + seed)
        assert total > 9 and mcux % 2
        for label, ri, fill in (("ri1", 1, 0), ("ri2_splits_rows", 2, 1), ("ri_row", mcux, 3), ("ri_total", total, 0),
                                ("ri_beyond", total + 7, 1), ("dri0", 0, 0), ("ri1_fill3", 1, 3)):
            out.append(("d/%s/%s/seed%d" % (sampling, label, seed), write(W, H, sampling, comps, quant, huff, ri=ri, fill=fill)))
        # the last block of every MCU ends in ten 1-bits (coefficient 63 = 1023, no EOB): with the 1-bit padding the last entropy
        # byte of every segment is 0xFF, stuffed
        tail = [c.copy() for c in comps]
        one = {0: q[0], 1: np.ones(64, np.int64)} if nc == 3 else {0: np.ones(64, np.int64)}
        last = tail[-1]
        last *= 0 if nc == 3 else 1
        if nc == 1:
            last[...] = np.sign(last) * np.minimum(np.abs(last), 20)          # the quantiser is 1 now; values stay small
        if nc == 3 or hs * vs == 1:
            last[..., 63] = 1023
        s = write(W, H, sampling, tail, one, huff, comp_q=(0, 1, 1)[:nc], ri=1, fill=seed % 2)
        out.append(("d/%s/stuffed_tail/seed%d" % (sampling, seed), s))
    return out


def stuffed_tails(stream):
    """how many entropy segments of the stream end in a stuffed 0xFF (mjpeg_ref counts the fill bytes before RSTn to the segment)"""
    return sum(seg.rstrip(b"\xff").endswith(b"\xff\x00") for seg in ref.parse(stream, ref.std_tables()).segments)


def checkerboard(W, H, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    period = int(rng.integers(1, 4))
    c = (((x // period + y // period) & 1) * 255).astype(np.uint8)
    return np.stack([c, 255 - c if seed & 1 else c, np.roll(c, 1, 1)], -1)


def class_e(seed):
    """encoder-like content with random quantisers 1-255"""
    rng = np.random.default_rng(400 + seed)
    out = []
    for name, make in (("noise", lambda W, H: rng.integers(0, 256, (H, W, 3), dtype=np.uint8)),
                       ("checker", lambda W, H: checkerboard(W, H, seed)), ("texture", lambda W, H: _texture(W, H, 80 + seed))):
        for sampling, (W, H) in zip(SAMPLINGS, ((33, 17), (24, 16), (49, 19), (35, 33))):
            q = [_random_quant(rng) for _ in range(3)]
            comps = _encoded(make(W, H), sampling, [q[0], q[1], q[2]])
            huff = None if name == "texture" else tables(PROFILES[(seed + len(out)) % 3], 500 + seed,
                                                         ids=[(c, i) for c in (0, 1) for i in range(3)])
            nc = SAMPLINGS[sampling][0]
            kw = dict(comp_q=(0, 1, 2)[:nc], comp_h=((0, 0), (1, 1), (2, 2))[:nc]) if huff else dict(comp_q=(0, 1, 1)[:nc])
            quant = {0: q[0], 1: q[1], 2: q[2]} if huff else {0: q[0], 1: q[1]}
            if not huff:
                comps = _encoded(make(W, H), sampling, [q[0], q[1], q[1]])
            out.append(("e/%s/%s/seed%d" % (name, sampling, seed), write(W, H, sampling, comps, quant, huff, ri=(0, 3, 5)[seed % 3], **kw)))
    return out


CLASSES = {"a": class_a, "b": class_b, "c": class_c, "d": class_d, "e": class_e}


def class_streams(letter, seeds=SEEDS):
    return [item for seed in seeds for item in CLASSES[letter](seed)]


# ---- frames chosen for the launch shapes of k_mjpeg_huff / k_mjpeg_idct ----------------------------------------------------------
def sparse_frame(W, H, sampling, seed, ri, fill=0, comment=b""):
    """a frame of random sparse blocks (a DC value and three AC values each, quantisers up to 9, generated tables)"""
    rng = np.random.default_rng(seed)
    q = [_random_quant(rng, 1, 10) for _ in range(2)]
    comps = []
    for c, (by, bx) in enumerate(grid(W, H, sampling)):
        b = np.zeros((by, bx, 64), np.int64)
        b[..., 0] = rng.integers(-100, 100, (by, bx))
        for _ in range(3):
            np.put_along_axis(b, rng.integers(1, 64, (by, bx, 1)), rng.integers(-40, 41, (by, bx, 1)), -1)
        comps.append(into_domain(b, q[min(c, 1)]))
    return write(W, H, sampling, comps, {0: q[0], 1: q[1]}, tables(PROFILES[seed % 3], seed), ri=ri, fill=fill, comment=comment)


def lanes_of(nseg):
    """launch_mjpeg's choice for the largest segment count of a call"""
    return 64 if nseg <= 64 else (128 if nseg <= 128 else 256)


# label: (W, H, sampling, restart interval) -> segments / blocks / first chroma block, see test_launch_shapes_are_what_they_claim
LAUNCH = {
    "64seg": (64, 64, "gray", 1),               # 64 segments: the last count served by 64 lanes; 64 blocks
    "65seg": (104, 40, "gray", 1),              # 65: the first served by 128 lanes
    "128seg": (128, 64, "gray", 1),             # 128: the last served by 128 lanes
    "129seg": (344, 24, "gray", 1),             # 129: the first served by 256 lanes
    "256seg_256blocks": (256, 64, "gray", 1),   # one full trip of 256 lanes; exactly one full workgroup of k_mjpeg_idct
    "257seg_257blocks": (2056, 8, "gray", 1),   # lane 0 makes a second trip; block 256 is alone in the second workgroup
    "264seg": (264, 64, "gray", 1),
    "520seg": (520, 64, "gray", 1),             # lanes 0-7 make a third trip; three workgroups
    "cb_at_255": (120, 136, "1x1", 5),          # 15 x 17 MCUs: Cb starts at block 255, Cr at 510; 765 blocks, 51 segments
    "cb_at_256": (256, 64, "2x1", 3),           # 16 x 8 MCUs of two luma blocks: Cb at 256, Cr at 384; 512 blocks, 43 segments
    "cb_at_257": (2056, 8, "1x1", 2),           # 257 MCUs: Cb at 257, Cr at 514; 771 blocks, 129 segments
    "mix_1seg": (200, 96, "gray", 0),           # 25 x 12 MCUs in ONE segment ...
    "mix_300seg": (200, 96, "gray", 1),         # ... and in 300: one call holds both, its lanes follow the larger count
}


def launch_frames():
    return [(label, sparse_frame(W, H, sampling, 600 + i, ri, fill=i % 2)) for i, (label, (W, H, sampling, ri)) in enumerate(LAUNCH.items())]


def residue_frames(W=40, H=24, sampling="2x1"):
    """sixteen frames of one size whose stream lengths take every residue mod 16 (a COM segment of the right length each)"""
    out = []
    for r in range(16):
        s = sparse_frame(W, H, sampling, 700 + r, ri=2)
        pad = (r - len(s) - 4) % 16
        s = sparse_frame(W, H, sampling, 700 + r, ri=2, comment=b"c" * (pad + 16))
        assert len(s) % 16 == r
        out.append(("len%%16=%d" % r, s))
    return out


# ---- the size sweep for J3 / J4 and the crop -----------------------------------------------------------------------------------
SWEEP_H = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17)


def sweep_cases():
    out = []
    for sampling in ("2x1", "2x2"):
        out += [(sampling, W, H) for W in range(1, 21) for H in SWEEP_H] + [(sampling, 33, 17), (sampling, 47, 31), (sampling, 49, 33)]
    for sampling in ("1x1", "gray"):
        out += [(sampling, W, H) for W in range(1, 21) for H in (1, 8, 9)]
    return out


def sweep_stream(sampling, W, H):
    """Random chroma with large steps between neighbouring samples on the whole padded grid (so that replication, interpolation,
    edges clamped at the true size and edges taken from the padding all give different bytes) over a quiet, blocky luma."""
    nc, hs, vs = SAMPLINGS[sampling]
    rng = np.random.default_rng([W, H, hs, vs, nc])
    g = grid(W, H, sampling)
    planes = [np.repeat(np.repeat(rng.integers(60, 200, (g[0][0] * 2, g[0][1] * 2)), 4, 0), 4, 1)]
    planes += [rng.choice([16, 70, 128, 190, 240], (by * 8, bx * 8)) + rng.integers(-12, 13, (by * 8, bx * 8)) for by, bx in g[1:]]
    q = [np.full(64, 2, np.int64), np.full(64, 3, np.int64)]
    comps = blocks_from_planes(planes, [q[0], q[1], q[1]][:nc])
    return write(W, H, sampling, comps, {0: q[0], 1: q[1]}, None, emit_dht=bool((W + H) & 1), ri=(W + H) % 3)
