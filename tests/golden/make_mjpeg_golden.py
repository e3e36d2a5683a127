"""Regenerates tests/golden/mjpeg_*.npz: baseline JPEG streams written by Pillow (libjpeg-turbo) and the RGB images the same
library decodes from them.  These pin the decoding rules J1-J5 to the real library; the tests read
the files only and do not need Pillow.

    python tests/golden/make_mjpeg_golden.py                  # the fixtures
    python tests/golden/make_mjpeg_golden.py --only NAME...   # some of them
    python tests/golden/make_mjpeg_golden.py --timing 32 DIR  # 32 + 32 1280x720 4:2:2 q85 streams (with / without restart
                                                              # intervals) for tools/time_mjpeg.py; DIR is not committed
"""
import io
import os
import sys

import numpy as np

try:
    from PIL import Image
except ImportError:           # the image generators below serve tests that run without Pillow
    Image = None

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mjpeg_ref  # noqa: E402

SUB = {"444": 0, "422": 1, "420": 2}
CORRUPT_SEED, CORRUPT_COUNT = mjpeg_ref.CORRUPT_SEED, mjpeg_ref.CORRUPT_COUNT   # test_mjpeg_cpu.py runs all; eight are stored


def texture(W, H, seed):
    """seeded texture plus noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    ph = rng.random(6) * 6.28
    base = np.stack([128 + 80 * np.sin(x * 0.31 + ph[c]) * np.cos(y * 0.23 + ph[c + 3]) for c in range(3)], -1)
    blocks = rng.integers(-40, 40, (H // 8 + 1, W // 8 + 1, 3)).repeat(8, 0).repeat(8, 1)[:H, :W]
    return np.clip(base + blocks + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)


def noise(W, H, seed):
    """black / white noise, a white, a black and a checkerboard block: the largest DC steps and AC values there are"""
    img = (np.random.default_rng(seed).integers(0, 2, (H, W, 1), dtype=np.uint8) * 255).repeat(3, 2)
    img[:8, :8], img[:8, 8:16] = 255, 0
    y, x = np.mgrid[0:8, 0:8]
    img[:8, 16:24] = (((x + y) & 1) * 255)[..., None]
    return img


def noise4(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def gradient(W, H, seed):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(W + H - 2, 1)], -1).astype(np.uint8)


def encode(img, sampling, quality, **opts):
    buf = io.BytesIO()
    if sampling == "gray":
        Image.fromarray(img[..., 1]).save(buf, "JPEG", quality=quality, **opts)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=SUB[sampling], **opts)
    return buf.getvalue()


def pillow_rgb(stream):
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))


def strip_dht(stream):
    b, out, p = bytes(stream), bytearray(b"\xff\xd8"), 2
    while b[p + 1] != 0xDA:
        L = (b[p + 2] << 8) | b[p + 3]
        if b[p + 1] != 0xC4:
            out += b[p:p + 2 + L]
        p += 2 + L
    return bytes(out + b[p:])


def dht_payload(stream):
    b, out, p = bytes(stream), b"", 2
    while b[p + 1] != 0xDA:
        L = (b[p + 2] << 8) | b[p + 3]
        if b[p + 1] == 0xC4:
            out += b[p + 4:p + 2 + L]
        p += 2 + L
    return out


# name: (W, H, sampling, quality, image, seed, options)
CASES = {
    "mjpeg_16x8_422_q75": (16, 8, "422", 75, texture, 1, {}),
    "mjpeg_1x1_420_q75": (1, 1, "420", 75, texture, 2, {}),
    "mjpeg_33x17_422_q90": (33, 17, "422", 90, texture, 3, {}),
    "mjpeg_50x34_420_q75_rstrows": (50, 34, "420", 75, texture, 4, dict(restart_marker_rows=1)),
    "mjpeg_97x65_422_q75_rst3": (97, 65, "422", 75, texture, 5, dict(restart_marker_blocks=3)),
    "mjpeg_40x24_444_q100_noise": (40, 24, "444", 100, noise, 6, {}),
    "mjpeg_64x48_gray_q50_opt": (64, 48, "gray", 50, texture, 7, dict(optimize=True)),
    "mjpeg_97x65_422_q30_opt": (97, 65, "422", 30, texture, 8, dict(optimize=True)),
    "mjpeg_96x64_422_q75_nodht": (96, 64, "422", 75, texture, 9, {}),
    "mjpeg_96x64_422_q75_gradient": (96, 64, "422", 75, gradient, 10, {}),
    "mjpeg_33x17_422_q90_corrupt": (33, 17, "422", 90, texture, 11, {}),
    # chroma planes of two columns: libjpeg replicates them instead of interpolating (J3)
    "mjpeg_4x5_420_q90_narrow": (4, 5, "420", 90, noise4, 12, {}),
    # more than 256 blocks (k_mjpeg_idct runs a second workgroup), and 264 / 65 / 23 entropy segments (k_mjpeg_huff with 256 lanes
    # and a second trip, with 128 lanes, with 64); in the 4:2:0 frame Cb starts inside the first workgroup, at block 180
    "mjpeg_264x64_gray_q50_rst1": (264, 64, "gray", 50, texture, 13, dict(restart_marker_blocks=1)),
    "mjpeg_200x40_422_q60_rst1": (200, 40, "422", 60, texture, 14, dict(restart_marker_blocks=1)),
    "mjpeg_137x73_420_q75_rst2": (137, 73, "420", 75, texture, 15, dict(restart_marker_blocks=2)),
}
for _i in range(5):
    CASES["mjpeg_97x65_422_q75_batch%d" % _i] = (97, 65, "422", 75, texture, 20 + _i, dict(restart_marker_blocks=3))


def fixtures(only=None):
    for name, (W, H, sampling, q, make, seed, opts) in CASES.items():
        if only and name not in only:
            continue
        stream = encode(make(W, H, seed), sampling, q, **opts)
        extra = {}
        if name.endswith("_nodht"):
            full = pillow_rgb(stream)
            stream = strip_dht(stream)
            assert b"\xff\xc4" not in stream and np.array_equal(pillow_rgb(stream), full)
        rgb = pillow_rgb(stream)
        if name.endswith("_corrupt"):
            todo = mjpeg_ref.corruptions(stream, CORRUPT_SEED, CORRUPT_COUNT)
            raising, quiet = [], []
            for pos, val in todo:
                try:
                    mjpeg_ref.decode(mjpeg_ref.corrupted(stream, pos, val))
                    quiet.append((pos, val))
                except ValueError:
                    raising.append((pos, val))
            pick = sorted(raising[:4] + quiet[:8 - len(raising[:4])])
            extra = dict(corrupt_pos=np.array([p for p, _ in pick], np.int32), corrupt_val=np.array([v for _, v in pick], np.uint8))
            print("  corruptions: %d of %d are refused by mjpeg_ref; stored %s" % (len(raising), len(todo), pick))
        assert np.array_equal(mjpeg_ref.decode(stream, None if b"\xff\xc4" in stream else std_tables()), rgb), name
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, stream=np.frombuffer(stream, np.uint8), rgb=rgb, **extra)
        assert os.path.getsize(path) < 48 * 1024, name
        print(name, len(stream), "bytes of stream,", os.path.getsize(path), "bytes of file")
    if only:
        return
    # what the refusal tests and the default-table test need: a progressive stream, and the DHT payload of a plain stream
    img = texture(16, 8, 30)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=75, progressive=True)
    np.savez_compressed(os.path.join(HERE, "mjpeg_aux.npz"), progressive=np.frombuffer(buf.getvalue(), np.uint8),
                        std_dht=np.frombuffer(dht_payload(encode(img, "422", 75)), np.uint8))


def std_tables():
    """{(class, id): (bits, vals)} from the DHT payload of a non-optimised Pillow stream (the Annex K.3 tables)"""
    return mjpeg_ref.tables_from_dht(dht_payload(encode(texture(16, 8, 30), "422", 75)))


def timing(count, outdir):
    os.makedirs(outdir, exist_ok=True)
    for i in range(count):
        img = texture(1280, 720, 1000 + i)
        for tag, opts in (("rst", dict(restart_marker_rows=1)), ("norst", {})):
            with open(os.path.join(outdir, "%s_%03d.jpg" % (tag, i)), "wb") as fh:
                fh.write(encode(img, "422", 85, **opts))
    print("wrote", 2 * count, "streams to", outdir)


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--timing":
        timing(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) >= 3 and sys.argv[1] == "--only":
        fixtures(sys.argv[2:])
    else:
        fixtures()
