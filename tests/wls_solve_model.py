"""k_wls_solve<NCH> (csrc/k_wls.hip) restated lane by lane in float32 NumPy, the bound its result
is held to, and the inputs tests/test_wls_solve_model_cpu.py and tests/test_gpu_wls_solver.py share.

The model runs whole waves: 64 lanes, 64 / NCH lines per wave, lane k of a line owns the chunk [k CH, k CH + m); every
__shfl of the kernel is an index into the lane axis, with the kernel's clamps and maskings, and a lane of a dead line runs
like the kernel's (empty chunk, identity equation).  Every operation is a single float32 operation in the kernel's order;
what the model does not share with the device is the contraction of a * b + c into one fused operation.

The bound.  A pass solves A u = f with A = I + lambda L, an M-matrix with unit row sums: A^-1 >= 0 with unit row sums, so
|A^-1|_inf = 1, max|u| <= max|f|, a later pass never amplifies an earlier pass's error in the maximum norm, and
cond_inf(A) <= 1 + 4 lambda w_max.  Hence for any sequence of passes

    max|u_dev - u_ref64| <= c * 2^-24 * max|f| * sum over the passes of (1 + 4 lambda_pass w_max).

`unit` is that expression without c; C_DEV_MAX is the c the device is held to: twice the larger of the model's and a float32
Thomas solve's c (tests/test_wls_solve_model_cpu.py measures both and asserts this value), rounded up to a power of two.  The
factor 2 is for the fused operations and the device's operation order.  Test infrastructure: the product never imports it."""
import numpy as np

import wls_ref as ref

C_DEV_MAX = 8.0
EPS = 2.0 ** -24

DEFECTS = ("drop_c_nY", "drop_c_nX", "chunk_len", "L_from_k", "cr_short")      # each breaks the bound by far
GUARDS = ("no_last_mask", "no_cr_identity")      # maskings that only ever replace a factor of an exact zero: see the CPU test

# the line lengths of the GPU tests: every NCH (4 up to 128, 8 up to 256, 16 up to 512, 32 up to 1024, 64 above), chunks of
# one element (1 ... 4), empty trailing chunks (5: chunks of 2, 2, 1, 0; 9: 3, 3, 3, 0; 513, 1025, 2049, 2113), CH 32 and 64
GPU_LENGTHS = (1, 2, 3, 4, 5, 9, 127, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 2113, 4095, 4096)
LAMBDAS = (0.0, 0.25, 47.0, 3047.0, 50000.0)            # of the pass


def wls_nch(n):
    for nch in (4, 8, 16, 32):
        if (n + nch - 1) // nch <= 32:
            return nch
    return 64


def solve(F, wt, lam, defect=None):
    """launch_solve: F (nlines, len, 2) float32, wt (nlines, len) float32 with wt[:, j] between j - 1 and j (wt[:, 0] is never
    read), lam a float32 or one per line -> the solved F.  defect: one of DEFECTS or GUARDS, a deliberately changed kernel."""
    assert defect is None or defect in DEFECTS + GUARDS
    f32 = np.float32
    F = np.asarray(F, f32)
    wt = np.asarray(wt, f32)
    nlines, n = wt.shape
    nch = wls_nch(n)
    lpw = 64 // nch
    CH = (n + nch - 1) // nch
    nw = (nlines + lpw - 1) // lpw
    lane = np.arange(64)[None, :].repeat(nw, 0)
    wave = np.arange(nw)[:, None].repeat(64, 1)
    k = lane % nch
    line = wave * lpw + lane // nch
    live = line < nlines
    ln = np.where(live, line, 0)
    lamv = np.broadcast_to(np.asarray(lam, f32), (nlines,))[ln]
    s = k * CH
    e = np.where(live, np.minimum(s + (CH - 1 if defect == "chunk_len" else CH), n), s)
    m = e - s
    out = F.copy()
    zero, one = np.zeros((nw, 64), f32), np.ones((nw, 64), f32)

    def w(j):
        ok = (j > 0) & (j < n)
        return np.where(ok, wt[ln, np.clip(j, 0, n - 1)], f32(0))

    def fv(j):
        v = F[ln, np.clip(j, 0, n - 1)]
        return v[..., 0], v[..., 1]

    def shfl(v, src):
        return np.take_along_axis(v, src, 1)

    with np.errstate(all="ignore"):
        # 1. forward elimination of the interior
        cp, d1, d2, yp = zero, zero, zero, zero
        wprev = np.where(m > 0, w(s), f32(0))
        sc = np.zeros((max(CH - 1, 1), 4, nw, 64), f32)
        for i in range(CH - 1):
            j = s + i
            act = j < e - 1
            wn = w(j + 1)
            a, c = -lamv * wprev, -lamv * wn
            b = f32(1) - a - c
            f1, f2 = fv(j)
            inv = f32(1) / (b - a * cp)
            nyp = -a * (one if i == 0 else yp) * inv
            ncp = c * inv
            nd1 = (f1 - a * d1) * inv
            nd2 = (f2 - a * d2) * inv
            cp, d1, d2, yp = (np.where(act, x, y) for x, y in ((ncp, cp), (nd1, d1), (nd2, d2), (nyp, yp)))
            sc[i] = np.where(act, np.stack([cp, d1, d2, yp]), sc[i])
            wprev = np.where(act, wn, wprev)
        # 2. the chunk's reduced equation
        two = m >= 2
        lX1, lX2, lY, lZ = np.where(two, d1, zero), np.where(two, d2, zero), np.where(two, yp, one), np.where(two, -cp, zero)
        fX1, fX2, fY, fZ = lX1, lX2, np.where(two, yp, zero), np.where(two, -cp, one)
        for i in range(CH - 3, -1, -1):
            act = two & (i <= m - 3)
            vx, vy, vz, vw = sc[i]
            fX1, fX2, fY, fZ = (np.where(act, x, y) for x, y in ((vy - vx * fX1, fX1), (vz - vx * fX2, fX2),
                                                                 (vw - vx * fY, fY), (-vx * fZ, fZ)))
        nx = np.minimum(lane + 1, 63)
        nX1, nX2, nY, nZ = shfl(fX1, nx), shfl(fX2, nx), shfl(fY, nx), shfl(fZ, nx)
        if defect != "no_last_mask":
            last = k == nch - 1
            nX1, nX2, nY, nZ = (np.where(last, zero, x) for x in (nX1, nX2, nY, nZ))
        has = m >= 1
        wn = w(e)
        a, c = -lamv * wprev, -lamv * wn
        b = f32(1) - a - c
        f1, f2 = fv(e - 1)
        A = np.where(has, a * lY, zero)
        B = np.where(has, a * lZ + b if defect == "drop_c_nY" else a * lZ + b + c * nY, one)
        Cc = np.where(has, c * nZ, zero)
        if defect == "drop_c_nX":
            nX1, nX2 = zero, zero
        R1 = np.where(has, f1 - a * lX1 - c * nX1, zero)
        R2 = np.where(has, f2 - a * lX2 - c * nX2, zero)
        # cyclic reduction of the line's NCH equations
        st = 1
        while st < (nch // 2 if defect == "cr_short" else nch):
            lm, lp = np.maximum(lane - st, 0), np.minimum(lane + st, 63)
            Am, Bm, Cm, R1m, R2m = (shfl(x, lm) for x in (A, B, Cc, R1, R2))
            Ap, Bp, Cp, R1p, R2p = (shfl(x, lp) for x in (A, B, Cc, R1, R2))
            if defect != "no_cr_identity":
                lo, hi = k < st, k + st >= nch
                Am, Bm, Cm, R1m, R2m = (np.where(lo, i_, x) for x, i_ in ((Am, zero), (Bm, one), (Cm, zero), (R1m, zero), (R2m, zero)))
                Ap, Bp, Cp, R1p, R2p = (np.where(hi, i_, x) for x, i_ in ((Ap, zero), (Bp, one), (Cp, zero), (R1p, zero), (R2p, zero)))
            al, ga = -A / Bm, -Cc / Bp
            nA, nC = al * Am, ga * Cp
            nB = B + al * Cm + ga * Ap
            R1 = R1 + al * R1m + ga * R1p
            R2 = R2 + al * R2m + ga * R2p
            A, B, Cc = nA, nB, nC
            st <<= 1
        U1, U2 = R1 / B, R2 / B
        pv = lane if defect == "L_from_k" else np.maximum(lane - 1, 0)
        L1, L2 = shfl(U1, pv), shfl(U2, pv)
        L1, L2 = np.where(k == 0, zero, L1), np.where(k == 0, zero, L2)
        # 3. back substitution
        u1, u2 = U1, U2
        sel = has & live
        out[ln[sel], (e - 1)[sel]] = np.stack([u1[sel], u2[sel]], 1)
        for i in range(CH - 2, -1, -1):
            act = has & (i <= m - 2)
            vx, vy, vz, vw = sc[i]
            u1 = np.where(act, vy + vw * L1 - vx * u1, u1)
            u2 = np.where(act, vz + vw * L2 - vx * u2, u2)
            out[ln[act], (s + i)[act]] = np.stack([u1[act], u2[act]], 1)
    return out


def thomas(wt, lam, f, dtype):
    """One pass by the Thomas algorithm in `dtype`: wt (N, L), lam a scalar or (N,), f (N, L, K)."""
    wt = np.asarray(wt, dtype).copy()
    wt[:, 0] = 0
    lam = np.broadcast_to(np.asarray(lam, dtype), (wt.shape[0],))[:, None]
    a = -lam * wt
    c = np.zeros_like(a)
    c[:, :-1] = a[:, 1:]
    b = dtype(1) - a - c
    f = np.asarray(f, dtype)
    N, L = b.shape
    cp = np.empty((N, L), dtype); dp = np.empty(f.shape, dtype)
    cp[:, 0] = c[:, 0] / b[:, 0]
    dp[:, 0] = f[:, 0] / b[:, 0, None]
    for j in range(1, L):
        den = b[:, j] - a[:, j] * cp[:, j - 1]
        cp[:, j] = c[:, j] / den
        dp[:, j] = (f[:, j] - a[:, j, None] * dp[:, j - 1]) / den[:, None]
    u = np.empty(f.shape, dtype)
    u[:, L - 1] = dp[:, L - 1]
    for j in range(L - 2, -1, -1):
        u[:, j] = dp[:, j] - cp[:, j, None] * u[:, j + 1]
    return u


def ref64(wt, lam, f):
    """One pass in float64 by wls_ref.thomas, the float32 inputs (lam one float32 per line or a scalar) taken exactly."""
    wt = np.asarray(wt, np.float64).copy()
    wt[:, 0] = 0
    lam = np.broadcast_to(np.asarray(lam, np.float64), (wt.shape[0],))[:, None]
    a, b, c = ref.pass_matrices(wt, lam)
    return ref.thomas(a, b, c, np.asarray(f, np.float64))


def unit(wt, lam, f):
    """2^-24 max|f| (1 + 4 lambda w_max) per line and right-hand side: (N, K).  wt[:, 0] does not count."""
    wt = np.asarray(wt, np.float64)
    wmax = wt[:, 1:].max(1) if wt.shape[1] > 1 else np.zeros(wt.shape[0])
    lam = np.broadcast_to(np.asarray(lam, np.float64), (wt.shape[0],))
    return EPS * np.abs(np.asarray(f, np.float64)).max(1) * (1.0 + 4.0 * lam * wmax)[:, None]


def c_of(u, want, wt, lam, f):
    """the largest error of u against want in units of `unit`, per line: (N,)"""
    err = np.abs(np.asarray(u, np.float64) - want).max(1)
    un = unit(wt, lam, f)
    return np.where(err == 0, 0.0, err / np.where(un > 0, un, 1.0)).max(1)


# ---- right-hand sides --------------------------------------------------------------------------------------------------------
MIN_D, NUM_D = -4, 256                                   # the invalid value is -80; the data run from -64 to 4000
def disparities(rng, nlines, n, first_step=False):
    """int16 (nlines, n): random disparities x16 in -64 ... 4000; every third line (from line 1, or from line 0) a step map
    with a small ramp"""
    d = rng.integers(-64, 4001, (nlines, n)).astype(np.int16)
    x = np.arange(n)
    for i in range(nlines):
        if (i + (1 if first_step else 0)) % 3 == 1:
            d[i] = 160 + 3200 * ((x // max(1, n // 3 + i)) % 2) + x % 5
    return d


# ---- guides whose weights have a known structure -------------------------------------------------------------------------------
# For a pass along the rows: the rows' levels alternate so that every vertical pair differs by at least VCUT in every channel and
# wv is exactly 0; along a row the level flips by VCUT at a cut (weight exactly 0) and the first channel carries noise.
VCUT = 170
STRUCTURES = {
    # name: (channels, sigma, noise amplitude, share of cuts)
    "flat": (1, 1.5, 0, 0.0),            # wh == 1
    "cuts": (1, 1.5, 0, 0.05),           # wh in {0, 1}
    "noisy": (3, 3.0, 20, 0.0),          # wh = exp(-n / 3), n = 0 ... 20: 1 down to 1.3e-3
    "noisy_cuts": (3, 3.0, 20, 0.05),    # the same with 5 % exact zeros
    "sigma10": (1, 10.0, 40, 0.0),       # one line only (nothing couples a single row or column to a neighbour)
}


def row_guide(rng, name, nlines, n):
    """uint8 (nlines, n) or (nlines, n, 3) -> wv == 0 (but for sigma10) and wh as STRUCTURES says; the same cuts in every row"""
    cn, sigma, noise, cuts = STRUCTURES[name]
    q = np.cumsum(rng.random(n) < cuts) % 2
    if cuts and n >= 4:
        q[n // 2:] = (q[n // 2:] + (q[n // 2] == q[n // 2 - 1])) % 2          # at least one cut, in the middle
    p = np.arange(nlines)[:, None] % 2
    g = np.repeat((VCUT * (p ^ q[None, :]))[:, :, None], cn, 2)
    if noise:
        g[:, :, 0] += rng.integers(0, noise + 1, (nlines, n))
    g = g.astype(np.uint8)
    return g[:, :, 0] if cn == 1 else g


def guide_weights(G, sigma):
    """(wh, wv) float32 of a whole-frame ROI by wls_ref"""
    H, W = G.shape[:2]
    wh, wv = ref.weights(G, ref.lut(sigma), (0, W, 0, H))
    return wh.astype(np.float32), wv.astype(np.float32)


def zero_weight_guide(rng, H, W):
    """uint8 (H, W): a checkerboard of 0 / 200 plus noise 0 ... 30: every neighbour pair differs by 140 or more"""
    y, x = np.mgrid[0:H, 0:W]
    return (200 * ((x + y) % 2) + rng.integers(0, 31, (H, W))).astype(np.uint8)


# ---- drawn solver parameters for the 2-D test -----------------------------------------------------------------------------------
def pass_lambdas(p):
    """W6: the lambda of every iteration as the device holds it: computed in double, rounded to float32 once per pass"""
    return [np.float32(l) for l in ref.lambdas(p)]


def says_something(p, w_max=1.0):
    """whether the bound at c = C_DEV_MAX stays at or below 2^-8 max|f| for these parameters (two passes per iteration)"""
    return sum(2 * (1.0 + 4.0 * float(l) * w_max) for l in pass_lambdas(p)) * EPS * C_DEV_MAX <= 2.0 ** -8


def drawn_sets(seed=5, count=24):
    """`count` solver parameter sets: lambda log-uniform in 0.1 ... 1e5, sigma log-uniform in 0.3 ... 30, 1 ... 16 iterations,
    attenuation in (0, 1], ROI offsets 0 ... 9"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        off = [int(v) for v in rng.integers(0, 10, 4)]
        out.append(dict(lambda_=float(10.0 ** rng.uniform(-1, 5)), sigma_color=float(10.0 ** rng.uniform(np.log10(0.3), np.log10(30))),
                        num_iter=int(rng.integers(1, 17)), attenuation=float(1.0 - rng.random()), lrc_thresh=24,
                        depth_discontinuity_radius=2, min_disparity=MIN_D, num_disparities=NUM_D, roi_left=off[0],
                        roi_right=off[1], roi_top=off[2], roi_bottom=off[3], use_confidence=0))
    return out


def fgs(f, wh, wv, p):
    """wls_ref.fgs with every pass's lambda rounded to float32 as W6 has it (wls_ref.lambdas keeps the double)"""
    u = f.astype(np.float64)
    for lam in pass_lambdas(p):
        a, b, c = ref.pass_matrices(wh, float(lam))
        u = ref.thomas(a, b, c, u)
        a, b, c = ref.pass_matrices(wv.T, float(lam))
        u = ref.thomas(a, b, c, u.transpose(1, 0, 2)).transpose(1, 0, 2)
    return u
