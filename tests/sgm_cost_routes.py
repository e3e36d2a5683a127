"""The rows of the StereoSGBM cost-route table ("SGM: cost routes") and one or more small device cases per row,
shared by test_sgm_cost_plan_cpu.py (every row by number, every case plans to its row, every case's expected frames are live,
different and not refused -- on the references alone), test_gpu_sgm_cost_routes.py (the cases on the device) and
tools/sgm_routes_run.py (the cases under a kernel trace)."""
import numpy as np

# number -> variant, as plan_sgm_cost names it: <form>_<sum>[_chk][_w3].  Rows 21 - 40 are rows 1 - 20 under MODE_SGBM_3WAY with
# blockSize > 1: the same kernels, then k_sgm_warm3 in the row's form.
PLAIN = ["bt8_fused", "bt8_box", "bt8_box_chk", "bt8_any_chk",
         "bt16g_fused", "bt16g_fused_chk", "bt16g_box", "bt16g_box_chk", "bt16g_any", "bt16g_any_chk",
         "bt16c_fused", "bt16c_fused_chk", "bt16c_box", "bt16c_box_chk", "bt16c_any_chk",
         "census_fused", "census_box", "census_box_chk", "census_any", "census_any_chk"]
ROWS = {i + 1: v for i, v in enumerate(PLAIN)}
ROWS.update({i + 21: v + "_w3" for i, v in enumerate(PLAIN)})
# what no call reaches: a u8 form never runs fused with a check; colour at R >= 7 always checks (279 * 15^2 passes 32767 on its
# own), and so does BT8 at R >= 9 on the odd windows a handle has (93 * 19^2; "bt8_any" exists at the even window 18 alone)
UNREACHABLE = ["bt8_fused_chk", "census_fused_chk", "bt16c_any"]

P1 = 600


class Case:
    """One device case of a row: frames of (D + cols) x H, cols ~ 20 columns of cost domain, and the matcher's knobs.  f16:
    rtdm_debug_sgm_cost16 is on; paths 3 comes in through setMode on a handle created with paths 5."""
    def __init__(self, row, D, bs, H=12, cols=21, P2=2400, cn=1, cap=0, census=None, paths=5, f16=0, noise=20):
        self.row, self.D, self.bs, self.H, self.W, self.P2, self.cn, self.cap = row, D, bs, H, D + cols, P2, cn, cap
        self.census, self.paths, self.f16, self.noise = census, paths, f16, noise
        self.name = "row%d_D%d_bs%d" % (row, D, bs)

    def frames(self, n=3):
        """n textured pairs, the right view the left one moved by 2, 5, 8 .. columns, each view with noise of its own"""
        out = []
        for i in range(n):
            rng = np.random.default_rng(7000 + 131 * self.row + 17 * self.D + self.bs + i)
            shift = 2 + 3 * i
            T = rng.integers(0, 256, (self.H, self.W + shift, self.cn)).astype(np.float64)
            T = (T + np.roll(T, 1, 1) + np.roll(T, -1, 1) + np.roll(T, 1, 0) + np.roll(T, -1, 0)) / 5
            two = [np.clip(T + rng.integers(-self.noise, self.noise + 1, T.shape), 0, 255).astype(np.uint8) for _ in range(2)]
            L, R = two[0][:, :self.W], two[1][:, shift:shift + self.W]
            out.append((L[:, :, 0].copy(), R[:, :, 0].copy()) if self.cn == 1 else (L.copy(), R.copy()))
        return out

    def params(self):
        return dict(numDisparities=self.D, blockSize=self.bs, P1=P1, P2=self.P2)

    def want(self, L, R, oracle):
        """the reference that owns the case's form and mode; raises where the device would refuse the frame"""
        kw = self.params()
        if self.paths == 3:
            import sgm_3way_ref
            return sgm_3way_ref.sgm_compute(L, R, preFilterCap=self.cap, census=self.census, **kw)
        if self.census:
            import sgm_census_ref
            return sgm_census_ref.sgm_compute(L, R, census=self.census, paths=self.paths, **kw)
        if self.paths == 4:
            import sgm_hh4_ref
            return sgm_hh4_ref.sgm_compute(L, R, preFilterCap=self.cap, **kw)
        if self.cn == 3 or self.cap > 15:
            import sgm_cn_ref
            return sgm_cn_ref.sgm_compute_cn(L, R, preFilterCap=self.cap, paths=self.paths, **kw)
        return oracle.sgm_compute(L, R, paths=self.paths, **kw)

    def plan_numbers(self):
        """the configuration sgm_cost_plan_host takes: D H blockSize P2 cn ftz kind cw ch paths force16"""
        cw, ch = self.census or (9, 7)
        return [self.D, self.H, self.bs // 2 * 2 + 1, max(self.P2, P1 + 1), self.cn, max(self.cap, 15) | 1, int(bool(self.census)), cw, ch,
                self.paths, self.f16]


BIG = 30000          # a P2 that turns the check on at a small window
CASES = [
    # ---- Birchfield-Tomasi, u8 (gray, ftzero <= 95)
    Case(1, 16, 3, paths=8), Case(1, 64, 7),
    Case(2, 48, 3), Case(2, 16, 9, paths=4), Case(2, 16, 17, H=20), Case(2, 272, 5, paths=8),
    Case(3, 16, 7, P2=BIG),                                  # the u8 form pushed off the fused kernel by a limit of 2767
    Case(4, 16, 19, H=24),
    # ---- u16 gray: rtdm_debug_sgm_cost16 at preFilterCap 0, or preFilterCap 97 (M = 257)
    Case(5, 16, 3, f16=1), Case(5, 64, 7, cap=97),
    Case(6, 32, 3, cap=97, P2=31000),
    Case(7, 16, 13, f16=1, H=16), Case(7, 48, 3, f16=1),
    Case(8, 16, 13, cap=97, H=16),
    Case(9, 16, 15, f16=1, H=20),
    Case(10, 16, 15, cap=97, H=20),
    # ---- colour (M = 279 at preFilterCap 0)
    Case(11, 16, 3, cn=3), Case(11, 64, 7, cn=3, paths=8),
    Case(12, 16, 3, cn=3, P2=31000),
    Case(13, 16, 9, cn=3), Case(13, 48, 3, cn=3),
    Case(14, 16, 13, cn=3, H=16),
    Case(15, 16, 15, cn=3, H=20),
    # ---- census (gray; M = cw ch - 1)
    Case(16, 16, 3, census=(9, 7)), Case(16, 64, 7, census=(5, 5), paths=8),
    Case(17, 16, 9, census=(9, 7)), Case(17, 16, 17, census=(7, 3), H=20), Case(17, 48, 3, census=(3, 3)), Case(17, 272, 5, census=(9, 5)),
    Case(18, 16, 17, census=(9, 7), P2=16000, H=20),
    Case(19, 16, 19, census=(9, 7), H=24),
    Case(20, 16, 19, census=(9, 7), P2=12000, H=24),
    # ---- MODE_SGBM_3WAY: H = 24 gives stripes 2 and 3 a first source row below row 0 up to blockSize 19, so k_sgm_warm3 has rows to
    # write in every case; at blockSize 13 and above b.pix cannot hold C' on these frames (6 R W1 > W H) and the handle allocates
    Case(21, 16, 3, H=24, paths=3), Case(22, 48, 5, H=24, paths=3), Case(23, 16, 7, H=24, paths=3, P2=BIG), Case(24, 16, 19, H=24, paths=3),
    Case(25, 32, 5, H=24, paths=3, f16=1), Case(26, 32, 3, H=24, paths=3, cap=97, P2=31000), Case(27, 16, 13, H=24, paths=3, f16=1),
    Case(28, 16, 13, H=24, paths=3, cap=97), Case(29, 16, 15, H=24, paths=3, f16=1), Case(30, 16, 15, H=24, paths=3, cap=97),
    Case(31, 16, 5, H=24, paths=3, cn=3), Case(32, 16, 3, H=24, paths=3, cn=3, P2=31000), Case(33, 16, 9, H=24, paths=3, cn=3),
    Case(34, 16, 13, H=24, paths=3, cn=3), Case(35, 16, 15, H=24, paths=3, cn=3),
    Case(36, 64, 7, H=24, paths=3, census=(9, 7)), Case(37, 16, 9, H=24, paths=3, census=(5, 7)),
    Case(38, 16, 17, H=24, paths=3, census=(9, 7), P2=16000), Case(39, 16, 19, H=24, paths=3, census=(9, 7)),
    Case(40, 16, 19, H=24, paths=3, census=(9, 7), P2=12000),
]
