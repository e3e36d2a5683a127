"""The synthetic MJPEG streams of mjpeg_synth.py without a GPU.  For every stream class: inside the domain (mjpeg_synth's
docstring); mjpeg_ref.decode equals what Pillow / libjpeg-turbo decodes, byte for byte; the host build of the device's
segment-decoding loop (tests/mjpeg_host.cpp) returns statuses 0 / 0 and the NumPy coefficients; the same under
-fsanitize=address,undefined exits 0.  The device is then held against mjpeg_ref.decode on the same streams
(test_gpu_mjpeg_synth.py), where Pillow is not needed."""
import collections
import io

import numpy as np
import pytest

import mjpeg_ref as ref
import mjpeg_synth as synth
from mjpeg_hostbuild import run_host

CLASSES = ["a", "b", "c", "d", "e", "launch", "residues"]


@pytest.fixture(scope="module")
def std():
    return ref.std_tables()


@pytest.fixture(scope="module")
def streams():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = (synth.launch_frames() if name == "launch" else synth.residue_frames() if name == "residues"
                           else synth.class_streams(name))
        return cache[name]
    return get


def _pillow(stream):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))


# ---- the writer's own tools -----------------------------------------------------------------------------------------------------
def test_generated_tables_are_legal_and_reach_every_length():
    used = collections.Counter()
    for symbols in (synth.AC_SYMBOLS, synth.DC_SYMBOLS, list(range(20))):
        for profile in ("flat", "boundary", "deep", "chain", "random"):
            for seed in range(4):
                bits, vals = synth.huffman_table(symbols, profile, seed)
                synth.check_table(bits, vals)
                assert sorted(vals) == sorted(symbols)
                if len(symbols) == 162:
                    used.update(l for l in range(1, 17) if bits[l - 1])
                if profile == "boundary":
                    assert bits[7] >= len(symbols) // 3 and bits[8] >= len(symbols) // 3         # exactly 8 and exactly 9 bits
                if profile == "deep":
                    assert bits[15] == max(bits) and (len(symbols) < 100 or bits[15] > len(symbols) // 2)
                if profile == "flat" and len(symbols) == 162:
                    assert bits[7] == 162                                                         # the look-up alone
    assert sorted(used) == list(range(1, 17))                     # 162-symbol tables with codes at every length between them
    bits, _ = synth.huffman_table(list(range(20)), "chain", 0)
    assert sum(1 for b in bits[:13] if b) == 13 and bits[15]
    bits, _ = synth.huffman_table(list(range(16)), [1] * 16, 0)
    assert all(bits)                                              # one table with a code at each of the sixteen lengths


def test_32_bit_idct_arithmetic_cannot_wrap_inside_the_domain():
    gain = synth.islow_gain()
    assert gain == 61214
    assert gain * synth.DOMAIN + 131072 < 2 ** 31 - 1


def test_forward_path_is_an_encoder(std):
    """blocks_from_image -> write -> decode gives the image back within what quantiser 1-3 and chroma subsampling cost"""
    y, x = np.mgrid[0:32, 0:48]
    img = np.stack([x * 255 // 47, y * 255 // 31, (x + y) * 255 // 78], -1).astype(np.uint8)
    q = [np.full(64, 1, np.int64), np.full(64, 3, np.int64)]
    for sampling in ("1x1", "2x1", "2x2"):
        s = synth.write(48, 32, sampling, synth.blocks_from_image(img, [q[0], q[1], q[1]], sampling), {0: q[0], 1: q[1]})
        assert np.abs(ref.decode(s).astype(int) - img).max() <= 6, sampling
    s = synth.write(48, 32, "gray", synth.blocks_from_image(img[..., 1], [q[0]], "gray"), {0: q[0]}, comp_q=(0,))
    assert np.abs(ref.decode(s)[..., 0].astype(int) - img[..., 1]).max() <= 1


def test_into_domain_scales_and_never_drops(std):
    rng = np.random.default_rng(9)
    q = rng.integers(1, 9, 64)
    b = rng.integers(-1023, 1024, (3, 4, 64))
    got = synth.into_domain(b, q)
    assert got.shape == b.shape and (got != 0).any(-1).all()                  # every block is still there, and not emptied
    s = synth.write(32, 24, "gray", [got], {0: q}, comp_q=(0,))
    before = synth.write(32, 24, "gray", [b], {0: q}, comp_q=(0,))
    assert max(synth.extent(before)) > synth.DOMAIN >= max(synth.extent(s))
    small = rng.integers(-5, 6, (2, 2, 64))
    assert np.array_equal(synth.into_domain(small, q), small)                 # what is inside is left alone


# ---- what the classes claim to contain --------------------------------------------------------------------------------------------
def test_class_a_codes_every_symbol():
    for seed in synth.SEEDS:
        logs = []
        items = synth.class_a(seed, logs)
        assert len(logs) == len(items) == 8
        for log in logs:
            assert {k for c, k in log if c == "ac"} == set(synth.AC_SYMBOLS) and len(synth.AC_SYMBOLS) == 162
            assert {k for c, k in log if c == "dc"} == set(range(12))
    # the generated tables put those symbols on both sides of the 8-bit look-up
    for profile in synth.PROFILES:
        lengths = synth.lengths_of(synth.tables(profile, 1)[(1, 0)])
        assert min(lengths.values()) <= 8 and max(lengths.values()) == 16
    assert {8, 9} <= set(synth.lengths_of(synth.tables("boundary", 1)[(1, 0)]).values())


def test_class_b_holds_the_block_shapes(std):
    for label, s in synth.class_b(1):
        f = ref.parse(s, std)
        z = [c.reshape(-1, 64)[:, ref.ZIGZAG] for c in ref.coefficients(f)]       # back to zigzag order
        for comp in z:
            nz = comp != 0
            assert (nz[:, 63] & nz[:, 1:63].any(1)).any(), label                  # coefficient 63 present beside others
            assert (nz[:, 63] & ~nz[:, :63].any(1)).any(), label                  # only coefficient 63
            assert (nz[:, 1:].all(1)).any(), label                                # all 63 AC
            assert (nz[:, 0] & ~nz[:, 1:].any(1)).any(), label                    # DC only
            assert (~nz[:, 1:52].any(1) & nz[:, 52]).any() and (~nz[:, :49].any(1) & nz[:, 49]).any(), label      # three ZRLs
        luma = ref.coefficients(f)[0][..., 0]
        assert 2047 in np.abs(np.diff(luma.reshape(-1))) or f.hs * f.vs > 1, label
        if f.hs * f.vs == 4:                                                      # inside one MCU's four luma blocks
            assert any(abs(int(luma[0, 2 * m]) - int(luma[0, 2 * m + 1])) == 2047 for m in range(f.mcux)), label


def test_class_c_and_d_hold_what_their_labels_say(std):
    c = dict(synth.class_c(1))
    f = ref.parse(c["c/ids23/seed1"], std)
    assert sorted(f.qt) == [2, 3] and sorted(f.huff) == [(0, 2), (0, 3), (1, 2), (1, 3)]
    f = ref.parse(c["c/cbcr_differ/seed1"], std)
    assert f.comps[1][3] != f.comps[2][3] and f.scan[1][1:] != f.scan[2][1:] and f.huff[(1, 1)] != f.huff[(1, 2)]
    f = ref.parse(c["c/shared/seed1"], std)
    assert len(f.qt) == 1 and len(f.huff) == 2 and {x[1:] for x in f.scan} == {(0, 0)}
    assert b"\xff\xc4" not in c["c/no_dht/seed1"] and b"\xff\xc4" not in c["c/no_dht_gray/seed1"]
    assert c["c/packed/seed1"].count(b"\xff\xc4") == 1 and c["c/packed/seed1"].count(b"\xff\xdb") == 1
    assert c["c/separate/seed1"].count(b"\xff\xc4") == 4 and c["c/separate/seed1"].count(b"\xff\xdb") == 2
    assert np.array_equal(ref.decode(c["c/packed/seed1"]), ref.decode(c["c/separate/seed1"]))
    assert c["c/redefined/seed1"].count(b"\xff\xc4") == 8
    d = dict(synth.class_d(1))
    for sampling in synth.SAMPLINGS:
        s = d["d/%s/ri1/seed1" % sampling]
        n = len(ref.parse(s, std).segments)
        assert n > 9 and b"\xff\xd7\xff" not in s[:20] and s.count(b"\xff\xd0") >= 2            # the RST number wraps
        assert len(ref.parse(d["d/%s/ri_beyond/seed1" % sampling], std).segments) == 1
        assert ref.parse(d["d/%s/ri_beyond/seed1" % sampling], std).ri == n + 7
        assert b"\xff\xdd" not in d["d/%s/dri0/seed1" % sampling]
        assert b"\xff\xff\xff\xff\xd0" in d["d/%s/ri1_fill3/seed1" % sampling]
        tail = d["d/%s/stuffed_tail/seed1" % sampling]
        assert synth.stuffed_tails(tail) == len(ref.parse(tail, std).segments) == n, sampling


def test_launch_shapes_are_what_they_claim(std):
    shape = {label: synth.launch_shape(s, std) for label, s in synth.launch_frames()}
    assert [shape[k][0] for k in ("64seg", "65seg", "128seg", "129seg", "256seg_256blocks", "257seg_257blocks", "264seg", "520seg")] == \
        [64, 65, 128, 129, 256, 257, 264, 520]
    assert shape["256seg_256blocks"][1] == 256 and shape["257seg_257blocks"][1] == 257
    assert [shape[k][2][1] for k in ("cb_at_255", "cb_at_256", "cb_at_257")] == [255, 256, 257]
    assert (shape["mix_1seg"][0], shape["mix_300seg"][0]) == (1, 300)
    assert {synth.lanes_of(v[0]) for v in shape.values()} == {64, 128, 256}
    assert {-(-v[1] // 256) for v in shape.values()} == {1, 2, 3, 4}              # k_mjpeg_idct's gridDim.x
    assert sorted(len(s) % 16 for _, s in synth.residue_frames()) == list(range(16))


# ---- every class against the domain, the library and the host builds --------------------------------------------------------------
@pytest.mark.parametrize("name", CLASSES)
def test_streams_are_inside_the_domain(std, streams, name):
    for label, s in streams(name):
        assert max(synth.extent(s, std)) <= synth.DOMAIN, (label, synth.extent(s, std))


@pytest.mark.parametrize("name", CLASSES)
def test_numpy_rules_equal_pillow(std, streams, name):
    pytest.importorskip("PIL")
    for label, s in streams(name):
        want = _pillow(s)                                 # a stream the library refuses raises here: a finding, not a skip
        got = ref.decode(s, std)
        assert got.shape == want.shape and np.array_equal(got, want), (label, int((got != want).sum()))


@pytest.mark.parametrize("name", CLASSES)
def test_host_build_gives_the_numpy_coefficients(std, streams, tmp_path, name):
    for label, s in streams(name):
        run, recs = run_host(s, tmp_path)
        assert run.returncode == 0, label
        (pst, dst, coef), = recs
        want = np.concatenate([c.reshape(-1) for c in ref.coefficients(ref.parse(s, std))])
        assert (pst, dst) == (0, 0), label
        assert np.array_equal(coef.astype(np.int64), want), label


@pytest.mark.parametrize("name", CLASSES)
def test_sanitized_host_build_is_clean(streams, tmp_path, name):
    for label, s in streams(name):
        run, recs = run_host(s, tmp_path, sanitize=True)
        assert run.returncode == 0, label + run.stderr[-2000:]
        assert recs[0][:2] == (0, 0), label


def test_redefined_table_last_definition_wins_in_pillow_too(std):
    pytest.importorskip("PIL")
    for seed in synth.SEEDS:
        c = dict(synth.class_c(seed))
        a, b = c["c/redefined/seed%d" % seed], c["c/separate/seed%d" % seed]
        assert np.array_equal(_pillow(a), _pillow(b)) and np.array_equal(ref.decode(a), ref.decode(b))


# ---- the size sweep ---------------------------------------------------------------------------------------------------------------
def _planes(stream, std):
    f = ref.parse(stream, std)
    return f, [ref.idct(c) for c in ref.coefficients(f)]


def test_sweep_equals_pillow_and_stays_in_the_domain(std):
    pytest.importorskip("PIL")
    cases = synth.sweep_cases()
    assert len(cases) == 2 * 203 + 2 * 60
    for sampling, W, H in cases:
        s = synth.sweep_stream(sampling, W, H)
        assert max(synth.extent(s, std)) <= synth.DOMAIN
        got, want = ref.decode(s, std), _pillow(s)
        assert got.shape == (H, W, 3) and np.array_equal(got, want), (sampling, W, H, int((got != want).sum()))


def _interpolated(plane, W, H, hs, vs):
    """J3's general formulas WITHOUT the rule that planes of one or two columns are replicated"""
    n, m = -(-W // hs), -(-H // vs)
    c = plane[:m, :n].astype(np.int64)
    rows = [(c, c)] if vs == 1 else [(c, np.concatenate([c[:1], c[:-1]], 0)), (c, np.concatenate([c[1:], c[-1:]], 0))]
    out = np.empty((vs * m, 2 * n), np.int64)
    for par, (near, far) in enumerate(rows):
        s = near if vs == 1 else 3 * near + far
        left, right = ref._h2(s, n)
        out[par::vs, 0::2] = (3 * s + left + 1) >> 2 if vs == 1 else (3 * s + left + 8) >> 4
        out[par::vs, 1::2] = (3 * s + right + 2) >> 2 if vs == 1 else (3 * s + right + 7) >> 4
    return out[:H, :W]


def test_sweep_content_tells_the_upsampling_rules_apart(std):
    """Where J3's edge cases act, the sweep's content makes a wrong rule visible.  At n = 3 chroma columns (W = 5, 6), the first
    size that is interpolated, replicating changes the image; at n = 2 (W = 3, 4), the last that is replicated, interpolating
    does.  The neighbour past the TRUE size is clamped where the last output column (row) is an odd one, i.e. for even W (even H
    in 2x2) that is no multiple of the MCU: there, taking it from the padded plane changes the last column (row).  For odd W and
    odd H the last column (row) looks inwards and both rules give the same image -- by the formulas, so nothing is asserted."""
    for sampling in ("2x1", "2x2"):
        for W in (3, 4, 5, 6, 7, 12, 20):
            for H in synth.SWEEP_H:
                s = synth.sweep_stream(sampling, W, H)
                f, planes = _planes(s, std)
                y = planes[0][:H, :W]
                right = ref.decode(s, std)
                assert np.array_equal(right, ref.colour(y, *(ref.upsample(p, W, H, f.hs, f.vs) for p in planes[1:])))
                what = (sampling, W, H)
                if W <= 4:
                    other = ref.colour(y, *(_interpolated(p, W, H, f.hs, f.vs) for p in planes[1:]))
                    assert not np.array_equal(other, right), what
                    continue
                assert np.array_equal(right, ref.colour(y, *(_interpolated(p, W, H, f.hs, f.vs) for p in planes[1:])))
                replicated = ref.colour(y, *(np.repeat(np.repeat(p.astype(np.int64), f.vs, 0), f.hs, 1)[:H, :W] for p in planes[1:]))
                assert not np.array_equal(replicated, right), what
                padded = ref.colour(y, *(ref.upsample(p, p.shape[1] * f.hs, p.shape[0] * f.vs, f.hs, f.vs)[:H, :W] for p in planes[1:]))
                if W % 2 == 0 and W % 16:
                    assert not np.array_equal(padded[:, W - 1], right[:, W - 1]), what
                if f.vs == 2 and H % 2 == 0 and H % 16:
                    assert not np.array_equal(padded[H - 1], right[H - 1]), what
                if W % 2 and (f.vs == 1 or H % 2):
                    assert np.array_equal(padded, right), what


# ---- the damaged streams the device test compares images on ------------------------------------------------------------------------
def test_stored_corruptions_that_decode_stay_in_the_domain(std, tmp_path):
    """of the eight stored single-byte corruptions, those the host build (the device's loop) accepts and mjpeg_ref accepts are
    inside the domain: test_damaged_frame_between_two_good_ones compares the device's image of the damaged frame on them"""
    stream, _, z = ref.load_fixture("mjpeg_33x17_422_q90_corrupt")
    stored = list(zip(z["corrupt_pos"].tolist(), z["corrupt_val"].tolist()))
    run, recs = run_host(stream, tmp_path, corruptions=stored)
    assert run.returncode == 0
    compared = 0
    for (pos, val), (pst, dst, _) in zip(stored, recs):
        bad = ref.corrupted(stream, pos, val)
        try:
            ref.decode(bad, std)
        except ValueError:
            continue
        if (pst, dst) == (0, 0) and max(synth.extent(bad, std)) <= synth.DOMAIN:
            compared += 1
    assert compared >= 2
