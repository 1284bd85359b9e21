"""Address arithmetic of the halo weight gradient's lean pixel loop
(csrc/kernels/wgrad_halo.hip, LEAN) against the old loop's, in a NumPy model
of both: for every workgroup range, wave, lane and 64-pixel step the DMA byte
offsets of the dY rows and of the window pieces and the LDS bases of the B
fragments must be the same numbers.  The model follows the kernel line by
line (the plan, the lane decode, issue() / advance() and their lean_*
counterparts); it needs no GPU, so a slip in the carried scalars shows here
before a kernel runs with it."""
import numpy as np
import pytest

OOB = 0x80000000
M32 = 0xFFFFFFFF
NOROW = 0x40000000

# (N, H, W, C, OC, K, pad, groups): the cases of test_wgrad_halo_lean_gpu.py
SHAPES = {
    "conv3": (2, 13, 13, 256, 384, 3, 1, 1),
    "conv3_n1": (1, 13, 13, 256, 384, 3, 1, 1),
    "conv5": (5, 13, 13, 384, 256, 3, 1, 2),
    "conv4": (3, 13, 13, 384, 384, 3, 1, 2),
    "conv2": (2, 27, 27, 96, 256, 5, 2, 2),
    "wide": (2, 20, 20, 128, 128, 3, 1, 1),
    "vgg28": (2, 28, 28, 256, 256, 3, 1, 1),
    "s2d55": (2, 57, 57, 48, 96, 3, 0, 1),
    "vgg56": (1, 56, 56, 128, 256, 3, 1, 1),
    "vgg112": (1, 112, 112, 64, 128, 3, 1, 1),
    "vgg224": (1, 224, 224, 64, 64, 3, 1, 1),
}
# (var, MT, NP, KHT, KW, PB, seg), in the kernel's order of preference
CANDS = [(1, 128, 2, 3, 3, 7168, 0), (5, 128, 2, 3, 3, 7168, 1),
         (4, 128, 2, 3, 3, 10240, 0), (2, 96, 2, 3, 3, 7168, 0),
         (7, 96, 3, 3, 3, 8192, 1), (6, 64, 4, 3, 3, 7168, 1),
         (3, 128, 3, 1, 5, 5120, 0)]


def plan(shape, splits, pad=2):
    N, H, W, C, OC, K, p, groups = shape
    OH = OW = H + 2 * p - K + 1
    g = dict(N=N, H=H, W=W, C=C, OC=OC, OH=OH, OW=OW, KH=K, KW=K, pt=p, pl=p,
             Cg=C // groups, OCg=OC // groups, P=N * OH * OW, OHW=OH * OW)
    g["Wp"] = OW + max(pad, K - 1)
    span = (OW - 1 + 63) // OW + 1
    cross = 2 if g["OHW"] % 64 else 1
    spi = (g["OHW"] + 63) // 64
    dmax = 0
    for st in range(spi):
        pin = 64 * st
        last = min(pin + 63, g["OHW"] - 1)
        dmax = max(dmax, (last // OW - pin // OW) * g["Wp"] + last % OW -
                   pin % OW)
    for var, MT, NP, KHT, KW, PB, seg in CANDS:
        if K != KW or K % KHT or g["OCg"] % MT or g["Cg"] % (16 * NP):
            continue
        if seg:
            if spi * 64 * 100 > g["OHW"] * 103:
                continue
            if KHT * (dmax + K) * 32 > PB:
                continue
            g.update(SEGP=dmax + K, spi=spi, WR=0)
        else:
            WR = span + cross * (KHT - 1)
            if WR * g["Wp"] * 32 > PB:
                continue
            g.update(SEGP=0, spi=0, WR=WR)
        break
    else:
        raise AssertionError("no plan")
    tiles = groups * (g["OCg"] // MT) * (g["Cg"] // (16 * NP)) * (K // KHT)
    steps = N * spi if seg else (g["P"] + 63) // 64
    s = splits if splits > 0 else 512 // tiles
    s = max(1, min(s, steps))
    ks = (steps + s - 1) // s
    kspan = ks if seg else ks * 64
    return g, dict(MT=MT, NP=NP, KHT=KHT, PB=PB, SEG=bool(seg),
                   kgroups=K // KHT, kspan=kspan,
                   splits=(steps + ks - 1) // ks)


def a_sw(MT, r):
    if MT == 128:
        return r & 7
    if MT == 96:
        return (r >> 2) & 1
    return (r >> 1) & 3


class Lanes:
    """The lane invariants of wave w (both loops' setup code)."""

    def __init__(self, g, k, w, kh0, coff_x=16, coff_y=32):
        MT, NP, KHT, PB, SEG = k["MT"], k["NP"], k["KHT"], k["PB"], k["SEG"]
        lane = np.arange(64, dtype=np.int64)
        self.g, self.k, self.w, self.kh0 = g, k, w, kh0
        AP = MT * 2
        self.ABYTES = 64 * AP
        self.NAW = self.ABYTES // 1024 // 4
        self.NB = (NP * PB + 1023) // 1024
        self.NBW = (self.NB + 3) // 4
        self.STAGE = self.ABYTES + self.NB * 1024
        self.a_row, self.a_off = [], []
        for i in range(self.NAW):
            ib = (w * self.NAW + i) * 1024 + 16 * lane
            r = ib // AP
            pc = (ib - r * AP) >> 4
            lb = (pc >> 1) ^ a_sw(MT, r)
            m = lb * 16 + (pc & 1) * 8
            self.a_row.append(r)
            self.a_off.append(((r * g["OC"] + coff_y + m) * 2) & M32)
        WS = KHT * g["SEGP"] if SEG else g["WR"] * g["Wp"]
        self.b_rs, self.b_col, self.b_ok, self.b_j = [], [], [], []
        for i in range(self.NBW):
            pi = w + 4 * i
            ib = pi * 1024 + 16 * lane
            plane = ib // PB
            wb = ib - plane * PB
            slot = wb >> 5
            half = (wb >> 4) & 1
            base_ok = (pi < self.NB) & (plane < NP) & (slot < WS)
            if SEG:
                khs = slot // g["SEGP"]
                self.b_rs.append(khs)
                self.b_j.append(slot - khs * g["SEGP"])
                self.b_ok.append(base_ok)
                self.b_col.append(((coff_x + plane * 16 + half * 8) * 2) & M32)
            else:
                rs = slot // g["Wp"]
                cs = slot - rs * g["Wp"]
                iw = cs - g["pl"]
                self.b_rs.append(rs)
                self.b_j.append(np.zeros(64, dtype=np.int64))
                self.b_ok.append(base_ok & (cs < g["OW"] + g["KW"] - 1) &
                                 (iw >= 0) & (iw < g["W"]))
                self.b_col.append(((iw * g["C"] + coff_x + plane * 16 +
                                    half * 8) * 2) & M32)
        self.rowbytes = g["W"] * g["C"] * 2
        self.pixbytes = g["C"] * 2
        fr, fq = lane & 15, lane >> 4
        self.trp = fr & 3
        self.q = fq * 4 + (fr >> 2)
        # LEAN
        self.l_rs, self.l_bj, self.l_inv = [], [], []
        for i in range(self.NBW):
            if SEG:
                aj = self.b_j[i] // g["Wp"]
                bj = self.b_j[i] - aj * g["Wp"]
                r = self.b_rs[i] + aj
                self.l_bj.append(bj)
                self.l_rs.append(np.where(self.b_ok[i], r, NOROW))
                self.l_inv.append((r * self.rowbytes + (bj - g["pl"]) *
                                   self.pixbytes + self.b_col[i]) & M32)
            else:
                self.l_bj.append(self.b_j[i])
                self.l_rs.append(np.where(self.b_ok[i], self.b_rs[i], NOROW))
                self.l_inv.append((self.b_rs[i] * self.rowbytes +
                                   self.b_col[i]) & M32)
        self.l_b, self.l_k = [], []
        for i in range(4):
            c = self.q + 16 * i
            a = c // g["OW"]
            b = c - a * g["OW"]
            self.l_b.append(b)
            self.l_k.append((a * g["Wp"] + b) * 32 + self.trp * 8 +
                            self.ABYTES)


def live(L, i):
    return L.w + 4 * i < L.NB


def old_issue(L, n, pin, oh, ow, pend):
    g, k = L.g, L.k
    p = n * g["OHW"] + pin
    pa = (p * g["OC"] * 2) & M32
    plim = g["OHW"] - pin if k["SEG"] else pend - p
    out = [np.where(L.a_row[i] < plim, (pa + L.a_off[i]) & M32, OOB)
           for i in range(L.NAW)]
    if k["SEG"]:
        ihb = oh + L.kh0 - g["pt"]
        for i in range(L.NBW):
            if not live(L, i):
                continue
            sj = ow + L.b_j[i]
            rr = sj // g["Wp"]
            col = sj - rr * g["Wp"]
            ih = ihb + rr + L.b_rs[i]
            iw = col - g["pl"]
            ok = L.b_ok[i] & (col < g["OW"] + g["KW"] - 1) & (iw >= 0) & \
                (iw < g["W"]) & (ih >= 0) & (ih < g["H"])
            v = ((n * g["H"] + ih) * L.rowbytes + iw * L.pixbytes +
                 L.b_col[i]) & M32
            out.append(np.where(ok, v, OOB))
        return out
    rc = g["OH"] - oh + k["KHT"] - 1
    ih_a = oh + L.kh0 - g["pt"]
    ih_b = L.kh0 - g["pt"] - rc
    gr_a = n * g["H"] + ih_a
    gr_b = (n + 1) * g["H"] + ih_b
    n1ok = n + 1 < g["N"]
    for i in range(L.NBW):
        if not live(L, i):
            continue
        rs = L.b_rs[i]
        first = rs < rc
        ih = np.where(first, ih_a, ih_b) + rs
        gr = np.where(first, gr_a, gr_b) + rs
        ok = L.b_ok[i] & (ih >= 0) & (ih < g["H"]) & (first | n1ok)
        out.append(np.where(ok, (gr * L.rowbytes + L.b_col[i]) & M32, OOB))
    return out


def old_advance(g, SEG, n, pin, oh, ow):
    pin += 64
    if SEG and pin >= g["OHW"]:
        return n + 1, 0, 0, 0
    if not SEG and pin >= g["OHW"]:
        pin -= g["OHW"]
    ow += 64
    while ow >= g["OW"]:
        ow -= g["OW"]
        oh += 1
        if oh == g["OH"]:
            oh = 0
            n += 1
    return n, pin, oh, ow


def old_bb(L, cur, pin0, oh0, ow0):
    g, k = L.g, L.k
    kp = g["SEGP"] if k["SEG"] else g["Wp"]
    out = []
    for i in range(4):
        ow = ow0 + L.q + 16 * i
        gr = ow // g["OW"]
        owr = ow - gr * g["OW"]
        if k["SEG"]:
            slot = np.where(pin0 + L.q + 16 * i < g["OHW"],
                            gr * g["Wp"] + owr - ow0, 0)
        else:
            slot = (gr + np.where(oh0 + gr >= g["OH"], k["KHT"] - 1, 0)) * \
                g["Wp"] + owr
        base = cur + L.ABYTES + slot * 32 + L.trp * 8
        out += [base + kh * kp * 32 for kh in range(k["KHT"])]
    return out


class Lean:
    """LeanStep and the lean_* lambdas."""

    def __init__(self, L, n0, pin0, oh0, ow0, pend):
        g, SEG = L.g, L.k["SEG"]
        self.L = L
        self.n, self.pin, self.oh, self.ow = n0, pin0, oh0, ow0
        self.base = ((n0 * g["H"] + oh0 + L.kh0 - g["pt"]) * L.rowbytes +
                     (ow0 * L.pixbytes if SEG else 0)) & M32
        p = n0 * g["OHW"] + pin0
        self.pa = (p * g["OC"] * 2) & M32
        self.plim = g["OHW"] - pin0 if SEG else pend - p
        self.q64 = 64 // g["OW"]
        self.r64 = 64 - self.q64 * g["OW"]
        self.inc64 = (self.q64 * L.rowbytes +
                      (self.r64 * L.pixbytes if SEG else 0)) & M32
        self.inc_row = (L.rowbytes - (g["OW"] * L.pixbytes if SEG else 0)) & M32
        self.inc_img = ((g["H"] - g["OH"]) * L.rowbytes) & M32
        self.b_delta = ((g["H"] - g["OH"] - L.k["KHT"] + 1) * L.rowbytes) & M32
        self.b_lo = max(0, g["pt"] - L.kh0)
        self.b_len = max(0, g["H"] + g["pt"] - L.kh0 - self.b_lo)

    def copy(self):
        c = object.__new__(Lean)
        c.__dict__.update(self.__dict__)
        return c

    def issue(self):
        L, g, k = self.L, self.L.g, self.L.k
        if self.plim >= 64:
            out = [(self.pa + L.a_off[i]) & M32 for i in range(L.NAW)]
        else:
            out = [np.where(L.a_row[i] < self.plim,
                            (self.pa + L.a_off[i]) & M32, OOB)
                   for i in range(L.NAW)]
        nb_live = (L.NB - L.w + 3) >> 2
        if k["SEG"]:
            ihb = self.oh + L.kh0 - g["pt"]
            cw = max(0, min(g["W"], g["OW"] + g["KW"] - 1 - g["pl"]))
            wrapb = (L.rowbytes - g["Wp"] * L.pixbytes) & M32
            for i in range(L.NBW):
                if i == L.NBW - 1 and L.NB % 4 != 0 and not i < nb_live:
                    continue
                t = L.l_bj[i] + self.ow
                c = t >= g["Wp"]
                iw = (t - np.where(c, g["Wp"] + g["pl"], g["pl"])) & M32
                ih = (L.l_rs[i] + ihb + c) & M32
                a = (L.l_inv[i] + self.base + np.where(c, wrapb, 0)) & M32
                out.append(np.where((iw < cw) & (ih < g["H"]), a, OOB))
            return out
        rc = g["OH"] - self.oh + k["KHT"] - 1
        ih_a = self.oh + L.kh0 - g["pt"]
        a_lo = max(0, -ih_a)
        a_len = max(0, min(rc, g["H"] - ih_a) - a_lo)
        bl = rc + self.b_lo
        bn = self.b_len if self.n + 1 < g["N"] else 0
        base_b = (self.base + self.b_delta) & M32
        for i in range(L.NBW):
            if i == L.NBW - 1 and L.NB % 4 != 0 and not i < nb_live:
                continue
            rs = L.l_rs[i]
            v = np.where(((rs - bl) & M32) < bn, (L.l_inv[i] + base_b) & M32,
                         OOB)
            v = np.where(((rs - a_lo) & M32) < a_len,
                         (L.l_inv[i] + self.base) & M32, v)
            out.append(v)
        return out

    def advance(self):
        L, g, SEG = self.L, self.L.g, self.L.k["SEG"]
        self.pin += 64
        if SEG:
            if self.pin >= g["OHW"]:
                self.pa = (self.pa + self.plim * g["OC"] * 2) & M32
                self.pin = self.oh = self.ow = 0
                self.n += 1
                self.base = ((self.n * g["H"] + L.kh0 - g["pt"]) *
                             L.rowbytes) & M32
                self.plim = g["OHW"]
                return
        elif self.pin >= g["OHW"]:
            self.pin -= g["OHW"]
        self.pa = (self.pa + 64 * g["OC"] * 2) & M32
        self.plim -= 64
        self.oh += self.q64
        self.ow += self.r64
        self.base = (self.base + self.inc64) & M32
        if self.ow >= g["OW"]:
            self.ow -= g["OW"]
            self.oh += 1
            self.base = (self.base + self.inc_row) & M32
        if not SEG and self.oh >= g["OH"]:
            self.oh -= g["OH"]
            self.n += 1
            self.base = (self.base + self.inc_img) & M32

    def bb(self, cur):
        L, g, k = self.L, self.L.g, self.L.k
        kp = g["SEGP"] if k["SEG"] else g["Wp"]
        wp32 = g["Wp"] * 32
        thr = g["OW"] - self.ow
        dwp = (g["Wp"] - g["OW"]) * 32
        sb = cur + self.ow * 32
        wrap = cur + L.ABYTES + (g["OH"] - self.oh) * wp32
        out = []
        for i in range(4):
            base = L.l_k[i] + np.where(L.l_b[i] >= thr, dwp, 0)
            if k["SEG"]:
                base = np.where(L.q < self.plim - 16 * i, base,
                                L.trp * 8 + L.ABYTES) + cur
            else:
                base = base + sb
                base = base + np.where(base >= wrap, (k["KHT"] - 1) * wp32, 0)
            out += [base + kh * kp * 32 for kh in range(k["KHT"])]
        return out


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(x) & M32, np.asarray(y) & M32), \
            (what, i)


@pytest.mark.parametrize("splits", [0, 1, 7])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_lean_addresses_equal_old(name, splits):
    g, k = plan(SHAPES[name], splits)
    SEG = k["SEG"]
    total = g["N"] * g["spi"] if SEG else g["P"]
    ranges = sorted({0, min(1, k["splits"] - 1), k["splits"] // 2,
                     k["splits"] - 1})
    for kg in range(k["kgroups"]):
        for split in ranges:
            pbeg = split * k["kspan"]
            pend = min(total, pbeg + k["kspan"])
            assert pbeg < pend
            if SEG:
                n0 = pbeg // g["spi"]
                pin0 = (pbeg - n0 * g["spi"]) * 64
            else:
                n0 = pbeg // g["OHW"]
                pin0 = pbeg - n0 * g["OHW"]
            oh0 = pin0 // g["OW"]
            ow0 = pin0 - oh0 * g["OW"]
            nk = pend - pbeg if SEG else (pend - pbeg + 63) >> 6
            for w in range(4):
                L = Lanes(g, k, w, kg * k["KHT"])
                old = (n0, pin0, oh0, ow0)
                lc = Lean(L, n0, pin0, oh0, ow0, pend)
                _same(old_issue(L, *old, pend), lc.issue(), "first issue")
                nxt = old_advance(g, SEG, *old)
                ln = lc.copy()
                ln.advance()
                for kt in range(nk):
                    cur = (kt & 1) * L.STAGE
                    if kt + 1 < nk:
                        _same(old_issue(L, *nxt, pend), ln.issue(),
                              ("issue", kg, split, w, kt))
                    _same(old_bb(L, cur, old[1], old[2], old[3]), lc.bb(cur),
                          ("bb", kg, split, w, kt))
                    old = nxt
                    nxt = old_advance(g, SEG, *old)
                    lc = ln.copy()
                    ln.advance()
                    assert (lc.n, lc.oh, lc.ow) == (old[0], old[2], old[3])
