"""The float32 model of k_wls_solve (tests/wls_solve_model.py) against float64 Thomas, the constants of the bound the device
is held to, and the proof that the bound notices a wrong kernel: deliberate defects of the model on the GPU tests' own cases."""
import math

import numpy as np
import pytest

import wls_ref as ref
import wls_solve_model as M

LENGTHS = sorted(set(range(1, 261)) | {n + d for n in (512, 1024, 2048, 4096) for d in range(-2, 3)}
                 | {5, 130, 2049, 2113, 1026, 514})
WEIGHTS = ("random", "ones", "zeros5", "mixed")


def drawn_weights(rng, kind, n):
    if kind == "ones":
        return np.ones(n, np.float32)
    if kind == "mixed":
        return (10.0 ** rng.uniform(-3, 0, n)).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    if kind == "zeros5":
        w[rng.random(n) < 0.05] = 0
    return w


def lines_for(n, seed):
    """every lambda x every weight kind, one line each; right-hand side 0 int16 disparities, right-hand side 1 a step map"""
    rng = np.random.default_rng(seed * 7919 + n)
    wt, lam = [], []
    for l in M.LAMBDAS:
        for kind in WEIGHTS:
            wt.append(drawn_weights(rng, kind, n)); lam.append(l)
    wt, lam = np.stack(wt), np.array(lam, np.float32)
    N = len(lam)
    x = np.arange(n)[None, :]
    step = (160 + 3200 * ((x // max(1, n // 3)) % 2) + x % 5).repeat(N, 0)
    f = np.stack([rng.integers(-64, 4001, (N, n)), step], 2).astype(np.float32)
    return wt, lam, f


def test_nch_and_chunks():
    for n in range(1, 4097):
        nch = M.wls_nch(n)
        CH = (n + nch - 1) // nch
        assert nch in (4, 8, 16, 32, 64) and nch * CH >= n and CH <= (64 if n > 2048 else 32)
        assert nch == 4 or n > 32 * (nch // 2)
    assert [M.wls_nch(n) for n in (1, 128, 129, 256, 257, 512, 513, 1024, 1025, 4096)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    # The lengths at which trailing chunks are empty, n = q NCH + r with 0 < r and q + r < NCH: below 4 and at 5, 6, 9 for
    # NCH 4, never for NCH 8 and 16 (their lines have q >= 16), often for NCH 32 and 64.  The GPU list holds some for each.
    def empty(n):
        nch = M.wls_nch(n); CH = (n + nch - 1) // nch
        return nch - (n + CH - 1) // CH
    assert [empty(n) for n in (1, 2, 3, 4, 5, 9, 130, 513, 1025, 2049, 2113, 4096)] == [3, 2, 1, 0, 1, 1, 0, 1, 3, 1, 1, 0]
    assert not any(empty(n) for n in range(129, 513))
    assert {M.wls_nch(n) for n in M.GPU_LENGTHS if empty(n)} == {4, 32, 64}


def test_model_meets_the_bound_and_the_constant_follows():
    c_model = c_ref = 0.0
    per = {}
    for n in LENGTHS:
        wt, lam, f = lines_for(n, 1)
        want = M.ref64(wt, lam, f)
        cm = M.c_of(M.solve(f, wt, lam), want, wt, lam, f)
        cr = M.c_of(M.thomas(wt, lam, f, np.float32), want, wt, lam, f)
        for i, l in enumerate(lam):
            a = per.setdefault(float(l), [0.0, 0.0])
            a[0] = max(a[0], cm[i]); a[1] = max(a[1], cr[i])
        # a pass with lambda 0 returns its input bit for bit
        z = np.asarray(lam) == 0
        assert np.array_equal(M.solve(f, wt, lam)[z].view(np.int32), f[z].view(np.int32))
        c_model, c_ref = max(c_model, cm.max()), max(c_ref, cr.max())
    for l in sorted(per):
        print("lambda %-8g c_model %.3f  c_ref %.3f" % (l, per[l][0], per[l][1]))
    print("c_model %.3f  c_ref %.3f" % (c_model, c_ref))
    assert 2.0 ** math.ceil(math.log2(2 * max(c_model, c_ref))) == M.C_DEV_MAX


def test_zero_weights_and_single_elements_are_exact():
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 130, 257, 2113):
        f = rng.integers(-64, 4001, (3, n, 2)).astype(np.float32)
        got = M.solve(f, np.zeros((3, n), np.float32), np.float32(50000.0))
        assert np.array_equal(got.view(np.int32), f.view(np.int32))


def gpu_case(n, name, seed=0):
    """the GPU test's guide `name` at length n, 17 lines (one for sigma10) -> (wt, f)"""
    rng = np.random.default_rng(seed + n)
    sigma = M.STRUCTURES[name][1]
    nl = 1 if name == "sigma10" else 17
    wh, wv = M.guide_weights(M.row_guide(rng, name, nl, n), sigma)
    assert not wv.any()
    f = M.disparities(rng, nl, n).astype(np.float32)
    return wh, np.stack([f, np.ones_like(f)], 2)


def gpu_cases():
    for n in M.GPU_LENGTHS:
        for name in M.STRUCTURES:
            wt, f = gpu_case(n, name)
            for l in M.LAMBDAS[1:]:
                yield n, name, np.float32(l), wt, f


def worst_per_nch(defect, enough, longest=4096):
    """NCH -> (c, length, weights, lambda) of the defect's largest c on the GPU list, looking no further once c >= enough"""
    worst = {}
    for n, name, lam, wt, f in gpu_cases():
        nch = M.wls_nch(n)
        if n > longest or not worst.get(nch, (0.0,))[0] < enough:
            continue
        bad = M.solve(f, wt, lam, defect)
        c = M.c_of(bad[..., :1], M.ref64(wt, lam, f)[..., :1], wt, lam, f[..., :1]).max()
        if not c <= worst.get(nch, (0.0,))[0]:
            worst[nch] = (c, n, name, lam)
    for nch in sorted(worst):
        print("%s, NCH %d: c = %.3g at length %d, %s, lambda %g: %.3g x the bound" % ((defect, nch) + worst[nch] + (worst[nch][0] / M.C_DEV_MAX,)))
    return worst


@pytest.mark.parametrize("defect", [d for d in M.DEFECTS if d != "cr_short"])
def test_the_bound_notices_a_wrong_kernel(defect):
    """each defect misses the bound the device is held to (c <= C_DEV_MAX) by 100 x or more on a case of the GPU list, and that
    for every instantiation of the kernel"""
    worst = worst_per_nch(defect, 100 * M.C_DEV_MAX)
    for nch in (4, 8, 16, 32, 64):
        assert not worst[nch][0] < 100 * M.C_DEV_MAX


def test_a_short_cyclic_reduction_is_noticed_where_it_matters():
    """Without its last step the cyclic reduction leaves chunks NCH / 2 apart uncoupled.  For NCH 4 that misses the bound by
    10^4 x.  The more chunks a line has the less the step carries: chunks 16 x 17 elements and more apart are coupled by
    exp(-distance / sqrt(lambda)), which for every lambda at which the bound says anything is below the bound itself, and at
    lambda 50000 the bound is loose by the condition number.  So for NCH 32 and 64 a bound on the forward error sees this
    defect barely or not at all (measured c: 447, 188, 24, 8.9 for NCH 8 ... 64), and rightly: the result is that close."""
    worst = worst_per_nch("cr_short", np.inf, longest=1100)
    assert not worst[4][0] < 100 * M.C_DEV_MAX
    assert worst[8][0] > M.C_DEV_MAX and worst[16][0] > M.C_DEV_MAX


@pytest.mark.parametrize("guard", M.GUARDS)
def test_the_maskings_guard_exact_zeros(guard):
    """Two maskings of the kernel replace a factor whose partner is exactly zero, so dropping them changes no bit on any case of
    the GPU list: they are no defects the bound could or need notice (they keep an infinity or NaN of a neighbouring line out).
    - k == NCH - 1 (the next chunk's first-element expression): the last chunk that holds elements ends at the line's end, where
      c = -lambda w(len) = -0; what the shuffle brings in from the next line, a dead line or the lane itself is finite.
    - the identity padding of the cyclic reduction: chunk 0 starts at element 0 where a = -lambda w(0) = -0, so A(0) = 0, and by
      induction A(k) = 0 for k < st after every step, likewise C(k) = 0 for k + st >= NCH: al and ga are zero there."""
    for n, name, lam, wt, f in gpu_cases():
        if n > 600 and name != "noisy_cuts":
            continue
        assert np.array_equal(M.solve(f, wt, lam).view(np.int32), M.solve(f, wt, lam, guard).view(np.int32)), (n, name)


def test_the_guides_give_the_weights_the_gpu_tests_rely_on():
    t15, t3 = ref.lut(1.5), ref.lut(3.0)
    assert t15[0] == 1 and t3[0] == 1 and ref.lut(10.0)[0] == 1
    # one channel at sigma 1.5: a difference of 132 or more is exactly 0, 131 is not
    assert not t15[132 ** 2:].any() and t15[131 ** 2] > 0
    # three channels at sigma 3: two channels differ by VCUT and the noisy one by VCUT - 20 at the least
    assert not t3[2 * M.VCUT ** 2 + (M.VCUT - 20) ** 2:].any()
    rng = np.random.default_rng(0)
    for name, (cn, sigma, noise, cuts) in M.STRUCTURES.items():
        for nl, n in ((1, 4096), (17, 129), (3, 5)):
            if name == "sigma10" and nl > 1:
                continue
            wh, wv = M.guide_weights(M.row_guide(rng, name, nl, n), sigma)
            assert not wv.any()                                   # the other direction's pass is the identity
            inner = wh[:, 1:]
            if name == "flat":
                assert (inner == 1).all()
            elif name == "cuts":
                assert np.isin(inner, (0, 1)).all() and (inner == 0).any() and (inner == 1).any()
            else:
                assert inner.max() <= 1 and (inner.min() > 0) == (cuts == 0)
                if n > 100:
                    assert inner[inner > 0].min() < 3e-2 and inner.max() == 1
                    assert ((inner == 0).any()) == (cuts > 0)
    # the zero-weight guide of the GPU test: every neighbour pair differs by 132 or more
    g = M.zero_weight_guide(rng, 33, 257)
    wh, wv = M.guide_weights(g, 1.5)
    assert not wh.any() and not wv.any()
