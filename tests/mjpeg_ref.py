"""Baseline JPEG decoding restated in NumPy: rules J1-J5 of DESIGN.md section 4.12 (libjpeg's defaults: JDCT_ISLOW, fancy
upsampling).  test_mjpeg_cpu.py holds it against the images Pillow / libjpeg-turbo decoded from the fixtures (byte for byte),
which pins the rules to the library; the device and the host build of csrc/rtdm_mjpeg.h are then held against this file.

The parser here is deliberately independent of the C one (it raises ValueError where that one refuses)."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])


class Frame:
    pass


def _u16(b, p):
    return (b[p] << 8) | b[p + 1]


def parse(data, default_tables=None):
    """Headers of one baseline frame -> Frame (W, H, ncomp, hs, vs, ri, qt, huff, segments...).  default_tables: {(cls, id):
    (bits, vals)} used when the stream carries no DHT at all."""
    b = bytes(data)
    if b[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    f = Frame()
    f.qt, f.huff, f.ri, f.has_dht, f.comps = {}, {}, 0, False, None
    p = 2
    while True:
        if p >= len(b) or b[p] != 0xFF:
            raise ValueError("marker expected at %d" % p)
        while p < len(b) and b[p] == 0xFF:
            p += 1
        m = b[p]
        p += 1
        if m == 0xD9:
            raise ValueError("no SOS")
        L = _u16(b, p)
        seg = b[p + 2:p + L]
        if p + L > len(b):
            raise ValueError("segment runs past the end")
        if m == 0xC0:
            if seg[0] != 8:
                raise ValueError("precision")
            f.H, f.W, n = _u16(seg, 1), _u16(seg, 3), seg[5]
            f.comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(n)]
        elif 0xC0 < m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise ValueError("not baseline")
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                assert seg[q] >> 4 == 0
                f.qt[seg[q] & 15] = np.frombuffer(seg[q + 1:q + 65], np.uint8).astype(np.int64)
                q += 65
        elif m == 0xC4:
            f.has_dht = True
            q = 0
            while q < len(seg):
                bits = list(seg[q + 1:q + 17])
                n = sum(bits)
                f.huff[(seg[q] >> 4, seg[q] & 15)] = (bits, list(seg[q + 17:q + 17 + n]))
                q += 17 + n
        elif m == 0xDD:
            f.ri = _u16(seg, 0)
        elif m == 0xDA:
            ns = seg[0]
            assert ns == len(f.comps)
            f.scan = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            p += L
            break
        p += L
    if not f.has_dht:
        f.huff = dict(default_tables)
    f.ncomp = len(f.comps)
    f.hs, f.vs = (f.comps[0][1], f.comps[0][2]) if f.ncomp == 3 else (1, 1)
    # entropy segments: split at RSTn, stop at EOI
    f.segments, start, q = [], p, p
    while True:
        q = b.find(b"\xff", q)
        if q < 0 or q + 1 >= len(b):
            raise ValueError("no EOI")
        n = b[q + 1]
        if n == 0:
            q += 2
        elif n == 0xFF:
            q += 1
        elif 0xD0 <= n <= 0xD7:
            f.segments.append(b[start:q])
            q += 2
            start = q
        elif n == 0xD9:
            f.segments.append(b[start:q])
            break
        else:
            raise ValueError("marker %02x inside the scan" % n)
    f.mcux = -(-f.W // (8 * f.hs))
    f.mcuy = -(-f.H // (8 * f.vs))
    return f


class _Bits:
    def __init__(self, seg):
        self.d = seg.replace(b"\xff\x00", b"\xff")
        self.p = 0          # bit position

    def get(self, n):
        v = 0
        for _ in range(n):
            byte = self.d[self.p >> 3] if (self.p >> 3) < len(self.d) else 0
            v = (v << 1) | ((byte >> (7 - (self.p & 7))) & 1)
            self.p += 1
        return v


def _codes(bits, vals):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _symbol(br, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | br.get(1)
        if (length, code) in table:
            return table[(length, code)]
    raise ValueError("bad Huffman code")


def _extend(v, s):
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def coefficients(f):
    """J1: per component an array [blocks_y, blocks_x, 64] of dequantised coefficients in natural order (int64), the padded
    block grid of the interleaved scan (one component: ceil(W/8) x ceil(H/8))."""
    nc = f.ncomp
    fac = [(f.hs, f.vs)] + [(1, 1)] * (nc - 1)
    out = [np.zeros((f.mcuy * v, f.mcux * h, 64), np.int64) for h, v in fac]
    tabs = [(_codes(*f.huff[(0, td)]), _codes(*f.huff[(1, ta)])) for _, td, ta in f.scan]
    qts = [f.qt[c[3]] for c in f.comps]
    total = f.mcux * f.mcuy
    per = f.ri if f.ri else total
    assert len(f.segments) == -(-total // per)
    for si, seg in enumerate(f.segments):
        br = _Bits(seg)
        pred = [0] * nc
        for mcu in range(si * per, min(total, (si + 1) * per)):
            my, mx = divmod(mcu, f.mcux)
            for c in range(nc):
                h, v = fac[c]
                for j in range(v):
                    for i in range(h):
                        blk = out[c][my * v + j, mx * h + i]
                        s = _symbol(br, tabs[c][0])
                        pred[c] += _extend(br.get(s), s)
                        blk[0] = pred[c] * qts[c][0]
                        k = 1
                        while k < 64:
                            rs = _symbol(br, tabs[c][1])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise ValueError("coefficient index past 63")
                            blk[ZIGZAG[k]] = _extend(br.get(s), s) * qts[c][k]
                            k += 1
    return out


def _pass(x, shift, add):
    """one ISLOW pass along the last axis of x[..., 8]"""
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 - z3 * 15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (x[..., 0] + x[..., 4]) << 13
    tmp1 = (x[..., 0] - x[..., 4]) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    o = np.stack([t10 + tmp3, t11 + tmp2, t12 + tmp1, t13 + tmp0, t13 - tmp0, t12 - tmp1, t11 - tmp2, t10 - tmp3], -1)
    return (o + add) >> shift


def idct(coef):
    """J2 on [by, bx, 64] -> the component plane [by*8, bx*8] uint8"""
    by, bx, _ = coef.shape
    c = coef.reshape(by, bx, 8, 8).astype(np.int64)
    ws = _pass(c.transpose(0, 1, 3, 2), 11, 1024).transpose(0, 1, 3, 2)      # columns first
    px = np.clip(_pass(ws, 18, 131072) + 128, 0, 255)
    return px.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8).astype(np.uint8)


def _h2(row, n):
    """J3 horizontal step on int rows [..., n] -> (even, odd) weights applied by the caller"""
    left = np.concatenate([row[..., :1], row[..., :-1]], -1)
    right = np.concatenate([row[..., 1:], row[..., -1:]], -1)
    return left, right


def upsample(plane, W, H, hs, vs):
    """J3: a chroma plane (padded) -> [H, W].  n and m are the TRUE downsampled sizes.  Where n <= 2 libjpeg does not
    interpolate at all (jdsample.c asks for downsampled_width > 2): the samples are replicated."""
    n, m = -(-W // hs), -(-H // vs)
    c = plane[:m, :n].astype(np.int64)
    if hs == 1 and vs == 1:
        return c[:H, :W]
    if n <= 2:
        return np.repeat(np.repeat(c, vs, 0), hs, 1)[:H, :W]
    if vs == 1:
        left, right = _h2(c, n)
        out = np.empty((m, 2 * n), np.int64)
        out[:, 0::2] = (3 * c + left + 1) >> 2
        out[:, 1::2] = (3 * c + right + 2) >> 2
        return out[:H, :W]
    up = np.concatenate([c[:1], c[:-1]], 0)
    dn = np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * m, 2 * n), np.int64)
    for par, far in ((0, up), (1, dn)):
        s = 3 * c + far
        left, right = _h2(s, n)
        out[par::2, 0::2] = (3 * s + left + 8) >> 4
        out[par::2, 1::2] = (3 * s + right + 7) >> 4
    return out[:H, :W]


def colour(y, cb, cr):
    """J4"""
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data, default_tables=None):
    f = parse(data, default_tables)
    planes = [idct(c) for c in coefficients(f)]
    y = planes[0][:f.H, :f.W]
    if f.ncomp == 1:
        return np.repeat(y[..., None], 3, -1)
    return colour(y, upsample(planes[1], f.W, f.H, f.hs, f.vs), upsample(planes[2], f.W, f.H, f.hs, f.vs))


def entropy_range(data):
    """(first, last + 1) byte offsets of the entropy-coded data of a one-scan stream"""
    b = bytes(data)
    p = b.index(b"\xff\xda")
    return p + 2 + _u16(b, p + 2), b.rindex(b"\xff\xd9")


def corruptions(data, seed, count):
    """count single-byte corruptions (position, new value) inside the entropy data at seeded positions.  No 0xFF is made,
    removed or separated from the byte after it, so the marker structure -- what the host parser sees -- stays as it was and
    only the entropy decoder meets the damage."""
    b = bytes(data)
    lo, hi = entropy_range(b)
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        p = int(rng.integers(lo, hi))
        v = b[p] ^ int(rng.integers(1, 256))
        if b[p] == 0xFF or b[p - 1] == 0xFF or v == 0xFF:
            continue
        out.append((p, v))
    return out


def corrupted(data, pos, val):
    b = bytearray(data)
    b[pos] = val
    return bytes(b)


# ---- the stored fixtures (tests/golden/mjpeg_*.npz, written by tests/golden/make_mjpeg_golden.py) ----------------------------
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SINGLE = ["mjpeg_16x8_422_q75", "mjpeg_1x1_420_q75", "mjpeg_33x17_422_q90", "mjpeg_50x34_420_q75_rstrows",
          "mjpeg_97x65_422_q75_rst3", "mjpeg_40x24_444_q100_noise", "mjpeg_64x48_gray_q50_opt", "mjpeg_97x65_422_q30_opt",
          "mjpeg_96x64_422_q75_nodht", "mjpeg_96x64_422_q75_gradient", "mjpeg_33x17_422_q90_corrupt", "mjpeg_4x5_420_q90_narrow",
          "mjpeg_264x64_gray_q50_rst1", "mjpeg_200x40_422_q60_rst1", "mjpeg_137x73_420_q75_rst2"]
BATCH = ["mjpeg_97x65_422_q75_batch%d" % i for i in range(5)]
FIXTURES = SINGLE + BATCH                          # sixteen, the narrow frame that pins J3's replication rule, and three
                                                   # frames of more than 256 blocks with 264, 65 and 23 entropy segments
CORRUPT_SEED, CORRUPT_COUNT = 20240607, 64         # make_mjpeg_golden.py stores eight of these corruptions


def load_fixture(name):
    """-> (stream bytes, rgb H x W x 3 as Pillow decoded it, the npz)"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z["stream"].tobytes(), z["rgb"], z


def tables_from_dht(payload):
    """DHT payload(s) -> {(class, id): (bits, vals)}"""
    b, out, q = bytes(payload), {}, 0
    while q < len(b):
        bits = list(b[q + 1:q + 17])
        out[(b[q] >> 4, b[q] & 15)] = (bits, list(b[q + 17:q + 17 + sum(bits)]))
        q += 17 + sum(bits)
    return out


def std_tables():
    """the standard's typical tables, as libjpeg wrote them into the DHT of a non-optimised stream (stored fixture data)"""
    return tables_from_dht(np.load(os.path.join(GOLDEN, "mjpeg_aux.npz"))["std_dht"].tobytes())
