"""Shapes, inputs and references shared by the census edge tests (test_gpu_census_edges.py) and the
CPU check that they reach what they claim (test_census_cases_cpu.py).  Nothing here needs a GPU.

The census cost has two kernels of its own (csrc/sdr_census.hip).  k_census walks a row in steps of
its block (256 columns) and stages its seven rows four bytes a lane when the width, both strides
and the base are multiples of 4, a byte a lane otherwise.  k_cost_census<NR, K> has 12
instantiations, NR = blockSize in {1, 3, 5, 7, 9, 11}, K = 1 (D <= 128, column blocks of BCOLS = 32)
or 2 (D > 128, BCOLS = 16); a column block is an EDGE block when its box passes a border of the
matched columns and an interior block otherwise.  The tables below name what each entry reaches.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import census_ref as CR
from numpy_ref import SGM_3WAY, SGM_HH, SGM_HH4, SGM_SGBM, _box_rows
from stereo_depth_ruler_amd import synthetic as S
from test_plan_cpu import stripes_of

BLOCK_SIZES = (1, 3, 5, 7, 9, 11)
MODES = (SGM_SGBM, SGM_HH, SGM_3WAY, SGM_HH4)
KINDS = S.ADVERSARIAL_KINDS + ("ties", "ramps")


def p2_census_max(bs):
    """The largest P2 of the census cost domain, 2*P2 + 62*blockSize^2 <= 32767."""
    return (32767 - 62 * bs * bs) // 2


def kernel_of(bs, D):
    """(NR, K) of the k_cost_census instantiation a call takes."""
    return bs, 1 if D <= 128 else 2


def bcols_of(D):
    return 32 if D <= 128 else 16


def width_of(W1, minD, D):
    """The image width that leaves W1 matched columns."""
    return W1 - min(minD, 0) + max(minD + D, 0)


def census_loop(img):
    """sdr.h's descriptor as a plain loop over pixels and offsets, both clamps spelled out.  Tiny
    images only."""
    I = np.asarray(img)
    H, W = I.shape
    out = np.zeros((H, W), np.uint64)
    for y in range(H):
        for x in range(W):
            v, k = 0, 0
            for dy in range(-3, 4):
                for dx in range(-4, 5):
                    if dy == 0 and dx == 0:
                        continue
                    yy = min(max(y + dy, 0), H - 1)
                    xx = min(max(x + dx, 0), W - 1)
                    if int(I[yy, xx]) < int(I[y, x]):
                        v |= 1 << k
                    k += 1
            out[y, x] = v
    return out


# ---- inputs -------------------------------------------------------------------------------

def ties_pair(H, W, seed=0):
    """Three grey levels, 0 and 255 among them (most neighbours tie with the centre); the right
    image is the left one shifted by a few columns with about 10 % of its pixels redrawn."""
    rng = np.random.default_rng(seed)
    levels = np.array([0, 128, 255], np.uint8)
    s = int(rng.integers(1, 6))
    big = levels[rng.integers(0, 3, (H, W + s))]
    L = np.ascontiguousarray(big[:, :W])
    R = np.ascontiguousarray(big[:, s:s + W])
    redraw = rng.random((H, W)) < 0.1
    R[redraw] = levels[rng.integers(0, 3, int(redraw.sum()))]
    return L, R


def ramps_pair(H, W):
    """L = x, R = W-1-x: every descriptor is known (ramps_closed_form)."""
    assert W <= 256
    x = np.arange(W, dtype=np.uint8)
    return np.tile(x, (H, 1)), np.tile(x[::-1], (H, 1))


@lru_cache(maxsize=None)
def pair(kind, H, W, D=16, seed=0):
    """The input pair of a case (read-only, computed once)."""
    if kind == "ties":
        L, R = ties_pair(H, W, seed)
    elif kind == "ramps":
        L, R = ramps_pair(H, W)
    else:
        L, R = S.adversarial_pair(kind, H, W, D, seed=seed)
    L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


def ramps_closed_form(H, W, minD, D, bs, P2, mode):
    """(value, mask [H][W1][D]) of the ramps pair's cost volume, from the definition alone: a left
    pixel with four columns on its left has its 28 left neighbours darker, a right pixel with four
    columns on its right its 28 right ones, so pc = 56 wherever x and x - d both have four columns
    on either side, and C == P2 + 56 * blockSize^2 on every cell whose box lies there (the rows are
    identical, so the vertical clamps do not matter; MODE_HH's bottom rows keep P2 and are left
    out)."""
    maxD = minD + D
    minX1, W1 = max(maxD, 0), W + min(minD, 0) - max(maxD, 0)
    s = bs // 2
    x = minX1 + np.arange(W1)[:, None]
    d = minD + np.arange(D)[None, :]
    inner = (x >= 4) & (x <= W - 5) & (x - d >= 4) & (x - d <= W - 5)      # [W1][D]
    xi = np.clip(np.arange(W1)[:, None] + np.arange(-s, s + 1)[None, :], 0, W1 - 1)
    box_ok = inner[xi].all(1)                                             # [W1][D]
    mask = np.broadcast_to(box_ok, (H, W1, D)).copy()
    if mode in (SGM_HH, SGM_HH4):
        mask[max(1, H - s):] = False
    return P2 + 56 * bs * bs, mask


# ---- the transform ------------------------------------------------------------------------
# (name, H, W, layout): the matcher runs D = 16, blockSize 1, so W1 = W - 16 >= 1 is legal at
# every width.  Layouts: "dense" (stride W), ("stride", n) rows padded to W + n, "base1" both
# images one byte (mod 4: 1 and 3) into a flat buffer, ("batch", pad) three frames whose frame
# stride is H * W + pad.
TRANSFORM_SHAPES = [
    # W % 4 == 0, dense: the dword staging
    ("dword_20x7", 7, 20, "dense"),
    ("dword_256x3_one_trip", 3, 256, "dense"),
    ("dword_260x40_second_trip", 40, 260, "dense"),
    ("dword_1024x8_four_trips", 8, 1024, "dense"),
    # the byte staging, reached by an odd width
    ("odd_17x1", 1, 17, "dense"),
    ("odd_255x2", 2, 255, "dense"),
    ("odd_257x6_second_trip", 6, 257, "dense"),
    ("odd_515x8_third_trip", 8, 515, "dense"),
    # ... by a row stride that is no multiple of 4 on an aligned width
    ("stride1_20x2", 2, 20, ("stride", 1)),
    ("stride1_256x6", 6, 256, ("stride", 1)),
    ("stride7_260x3", 3, 260, ("stride", 7)),
    ("stride7_1024x1", 1, 1024, ("stride", 7)),
    # ... by a misaligned base on an aligned width and stride
    ("base1_20x8", 8, 20, "base1"),
    ("base1_256x40", 40, 256, "base1"),
    # three frames whose frame stride is no multiple of 4 (aligned width and rows), and dense odd
    ("batch_20x7_fstride142", 7, 20, ("batch", 2)),
    ("batch_260x2_fstride521", 2, 260, ("batch", 1)),
    ("batch_17x3_dense", 3, 17, ("batch", 0)),
]
TRANSFORM_KINDS = ("ties", "noise", "flat", "binary")
TRANSFORM_WIDTHS = {17, 20, 255, 256, 257, 260, 515, 1024}
TRANSFORM_HEIGHTS = {1, 2, 3, 6, 7, 8, 40}


def transform_layout(H, W, layout):
    """(frames, row stride, frame stride, byte offsets of the left and right base in one flat
    buffer, buffer bytes) of a TRANSFORM_SHAPES layout."""
    F, stride, pad, off = 1, W, 0, 0
    if layout == "base1":
        off = 1
    elif layout != "dense":
        what, n = layout
        if what == "stride":
            stride = W + n
        else:
            F, pad = 3, n
    fstride = H * stride + pad
    span = F * fstride
    offL = off
    offR = off + span + (2 if off else 0)  # base1: 1 and 3 (mod 4) when the span is a multiple of 4
    return F, stride, fstride, offL, offR, offR + span


def takes_dword_path(W, stride, fstride, base_mod4):
    """k_census's own condition for the four-bytes-a-lane staging."""
    return ((W | stride | fstride | base_mod4) & 3) == 0


# ---- the cost volume ----------------------------------------------------------------------

def _cost(name, bs, D, W1, H, mode, minD=0, kind="noise", P2=None, F=1):
    W = width_of(W1, minD, D)
    return SimpleNamespace(name=name, bs=bs, D=D, W1=W1, H=H, W=W, mode=mode, minD=minD, kind=kind,
                           P1=2 * bs * bs, P2=12 * bs * bs if P2 is None else P2, F=F, id=name)


def _pmax(bs):
    return p2_census_max(bs)


# Each entry's mode is the one the CPU checks run the whole pin in; the GPU test compares the cost
# volume of every entry under all four modes.  3*BCOLS + 5 holds one interior column block
# (blockSize <= 11: SW2 <= 5) between EDGE blocks.
COST_CASES = [
    # -- the 12 instantiations <NR, K>, with the W1 and D classes of each K spread over them
    _cost("k_1_1__W1_3bcols+5__D16", 1, 16, 101, 9, SGM_SGBM, kind="ties", P2=_pmax(1)),
    _cost("k_3_1__W1_bcols+1__D48", 3, 48, 33, 12, SGM_HH, kind="noise"),
    _cost("k_5_1__W1_bcols__D128", 5, 128, 32, 13, SGM_3WAY, kind="binary", P2=_pmax(5)),
    _cost("k_7_1__W1_bcols-1__D16__H37", 7, 16, 31, 37, SGM_HH4, kind="binary"),
    _cost("k_9_1__W1_3bcols+5__D48", 9, 48, 101, 23, SGM_SGBM, kind="noise", P2=_pmax(9)),
    _cost("k_11_1__W1_sw2+1__D128__H37", 11, 128, 6, 37, SGM_HH, kind="textured"),
    _cost("k_1_2__W1_3bcols+5__D144", 1, 144, 53, 8, SGM_HH, kind="ties"),
    _cost("k_3_2__W1_bcols+1__D256", 3, 256, 17, 11, SGM_3WAY, kind="noise", P2=_pmax(3)),
    _cost("k_5_2__W1_bcols__D144", 5, 144, 16, 10, SGM_HH4, kind="binary"),
    _cost("k_7_2__W1_bcols-1__D256__H37", 7, 256, 15, 37, SGM_SGBM, kind="noise", P2=_pmax(7)),
    _cost("k_9_2__W1_sw2+1__D144", 9, 144, 5, 20, SGM_3WAY, kind="ties"),
    _cost("k_11_2__W1_3bcols+5__D256", 11, 256, 53, 24, SGM_HH4, kind="noise", P2=_pmax(11)),
    # -- the narrowest frames of other block sizes
    _cost("W1_sw2+1__bs1_k1", 1, 16, 1, 6, SGM_HH, kind="noise"),
    _cost("W1_sw2+1__bs7_k1", 7, 48, 4, 9, SGM_3WAY, kind="ties"),
    _cost("W1_sw2+1__bs5_k2", 5, 256, 3, 7, SGM_SGBM, kind="noise"),
    # -- frame heights around the vertical window, blockSize 7 (SH2 = 3) and 11 (SH2 = 5)
    _cost("H_1__bs7", 7, 16, 40, 1, SGM_SGBM, kind="noise"),
    _cost("H_sh2__bs7", 7, 144, 20, 3, SGM_HH, kind="noise"),
    _cost("H_sh2+1__bs7", 7, 48, 37, 4, SGM_3WAY, kind="ties"),
    _cost("H_2sh2+1__bs7", 7, 16, 45, 7, SGM_HH4, kind="noise"),
    _cost("H_2sh2+2__bs7", 7, 144, 21, 8, SGM_HH, kind="binary"),
    _cost("H_1__bs11", 11, 144, 20, 1, SGM_HH, kind="noise"),
    _cost("H_sh2__bs11", 11, 16, 40, 5, SGM_3WAY, kind="noise"),
    _cost("H_sh2+1__bs11", 11, 48, 35, 6, SGM_HH4, kind="ties"),
    _cost("H_2sh2+1__bs11", 11, 144, 19, 11, SGM_SGBM, kind="noise"),
    _cost("H_2sh2+2__bs11", 11, 16, 43, 12, SGM_HH, kind="noise", P2=_pmax(11)),
    # -- the disparity range's position
    _cost("minD_3", 5, 48, 40, 14, SGM_SGBM, minD=3, kind="noise"),
    _cost("minD_-20__k2", 3, 144, 20, 9, SGM_3WAY, minD=-20, kind="ties"),
    _cost("minD_-20__k1", 9, 16, 37, 13, SGM_HH, minD=-20, kind="noise"),
    _cost("maxD_negative", 5, 16, 45, 12, SGM_SGBM, minD=-40, kind="noise"),
    _cost("maxD_negative__k2", 3, 144, 21, 7, SGM_HH4, minD=-200, kind="ties"),
    # -- inputs with a known or degenerate answer
    _cost("ramps__bs11_P2max", 11, 32, 88, 20, SGM_SGBM, kind="ramps", P2=_pmax(11)),
    _cost("ramps__k2_hh", 3, 144, 56, 9, SGM_HH, kind="ramps"),
    _cost("flat", 5, 48, 38, 9, SGM_SGBM, kind="flat"),
    _cost("periodic__k2", 5, 144, 37, 9, SGM_3WAY, kind="periodic"),
    _cost("steps", 9, 48, 70, 12, SGM_HH, kind="steps"),
    # -- batches: every frame is compared
    _cost("batch3__k1", 5, 48, 70, 11, SGM_3WAY, kind="noise", F=3),
    _cost("batch3__k2", 7, 144, 35, 9, SGM_HH, kind="ties", F=3),
]
COST_BY_ID = {c.id: c for c in COST_CASES}
W1_CLASSES = ("sw2+1", "bcols-1", "bcols", "bcols+1", "3bcols+5")
H_CLASSES = ("1", "sh2", "sh2+1", "2sh2+1", "2sh2+2", "37")


def w1_class(c):
    b, s = bcols_of(c.D), c.bs // 2
    return {s + 1: "sw2+1", b - 1: "bcols-1", b: "bcols", b + 1: "bcols+1", 3 * b + 5: "3bcols+5"}.get(c.W1)


def h_class(c):
    s = c.bs // 2
    return {1: "1", s: "sh2", s + 1: "sh2+1", 2 * s + 1: "2sh2+1", 2 * s + 2: "2sh2+2", 37: "37"}.get(c.H)


def cost_pairs(c):
    """The F input pairs of a cost case."""
    return [pair(c.kind, c.H, c.W, c.D, seed=1000 + 7 * f + len(c.name)) for f in range(c.F)]


def create_args(c, mode=None, uniq=12, d12=1, speckle=(0, 0)):
    """StereoSGBM.create's positional arguments of a case."""
    return (c.minD, c.D, c.bs, c.P1, c.P2, d12, 0, uniq, speckle[0], speckle[1], c.mode if mode is None else mode)


# ---- MODE_SGBM_3WAY stripes ---------------------------------------------------------------

def _stripe(H, W, D, bs, ns, kind="noise"):
    return SimpleNamespace(H=H, W=W, D=D, W1=W - D, bs=bs, ns=ns, kind=kind, minD=0, mode=SGM_3WAY,
                           P1=2 * bs * bs, P2=12 * bs * bs, F=1, id=f"{H}x{W}_d{D}_bs{bs}_ns{ns}_{kind}")


# the shapes of test_gpu_adversarial.test_3way_short_last_stripes: every row of the last stripes
# keeps its window clamped at the stripe start (aux_rows == end - s0)
SHORT_STRIPE_CASES = [_stripe(H, 90, 32, bs, ns) for bs in (7, 9, 11) for H in (14, 15, 17, 18, 21, 26)
                      for ns in (4, 8)]
STRIPE_CASES = SHORT_STRIPE_CASES + [
    _stripe(31, 70, 16, 5, 1, "ties"),       # one stripe: the frame, no band
    _stripe(31, 70, 16, 5, 3, "noise"),
    _stripe(31, 70, 16, 5, 4, "ties"),       # SH2 rows a band
    _stripe(31, 70, 16, 5, 8, "binary"),
    _stripe(33, 180, 144, 3, 3, "noise"),    # K = 2
    _stripe(26, 190, 144, 9, 8, "ties"),     # K = 2, short last stripes
    _stripe(9, 60, 16, 1, 4, "noise"),       # blockSize 1: SH2 = 0, no band holds a row
]


def horizontal_sums(L, R, minD, D, bs):
    """hs [H][W1][D]: the pixel cost summed over the box's columns, clamped to the matched ones."""
    pix = CR.census_pixel_cost(L, R, minD, D)
    W1, s = pix.shape[1], bs // 2
    xi = np.clip(np.arange(W1)[:, None] + np.arange(-s, s + 1)[None, :], 0, W1 - 1)
    return pix[:, xi, :].sum(2)


def stripe_rows_ref(L, R, minD, D, bs, P2, nstripes):
    """Stage 6's defined rows as [(stripe, rows [aux_rows][W1][D])] for the stripes that keep rows
    of their own, and the buffer's (stripes, rows a band).  Band s, rows [0, aux_rows) hold the
    stripe's first cost rows, the vertical window clamped at the stripe start s0; the rest of a
    band, and the band of a stripe that starts at row 0, are undefined."""
    H, SH2 = L.shape[0], bs // 2
    st = stripes_of(H, nstripes, bs, SH2)
    hs = horizontal_sums(L, R, minD, D, bs)
    out = [(s, P2 + _box_rows(hs, s0, s0 + aux, SH2, False)) for s, (s0, end, out0, aux) in enumerate(st) if aux]
    return out, (len(st), max(x[3] for x in st))


# ---- row bands ----------------------------------------------------------------------------
# k_cost_census and the BT cost's k_cost share one launch rule and one row loop: a block owns a band
# of TY rows and walks n = tlast - tfirst + 1 + 2 SH2 virtual rows in a loop unrolled by U = 2 NR,
# n // U full trips and a tail of n % U rows.  The launcher's own TY (the tallest band that fills the
# device in one pass, at least 4) gives every small frame 4-row bands; the debug knob
# SDR_DEBUG_COST_ROWS sets it instead.

def is_hh(mode):
    return mode in (SGM_HH, SGM_HH4)


BAND_CLASSES = ("n<U", "n==U", "n==U+1", "n==3U-1", "n>=3U", "short_last", "straddles_ylim", "frozen",
                "hh_straddles_yl", "hh_p2_only", "TY1", "one_band")
# blockSize 1 has no frozen and no P2 rows (SH2 = 0: ylim = H - 1, yl = H)
BAND_CLASSES_BS1 = tuple(c for c in BAND_CLASSES if c not in ("straddles_ylim", "frozen", "hh_straddles_yl",
                                                              "hh_p2_only"))

def band_shape(cls, nr):
    """(TY, H, mode) of the entry built for a band class: a band clear of the frozen rows walks
    n = TY + 2 SH2 = TY + NR - 1 virtual rows, and U = 2 NR."""
    s = nr // 2
    if cls == "n<U":
        ty = nr if nr > 1 else 1
        return ty, 3 * ty + s + 2, SGM_SGBM
    if cls in ("n==U", "n==U+1", "n==3U-1", "n>=3U"):
        ty = {"n==U": nr + 1, "n==U+1": nr + 2, "n==3U-1": 5 * nr, "n>=3U": 5 * nr + 3}[cls]
        return ty, ty + s + 3, SGM_3WAY if cls == "n==U+1" else SGM_SGBM
    if cls == "short_last":
        return 4, 13, SGM_SGBM
    if cls == "straddles_ylim":
        return s + 3, 2 * (s + 3), SGM_SGBM
    if cls == "frozen":
        return (1 if s == 1 else 2), 2 * s + 6, SGM_3WAY
    if cls == "hh_straddles_yl":
        return s + 2, 2 * (s + 2), SGM_HH
    if cls == "hh_p2_only":
        return 1, 2 * s + 4, SGM_HH4
    if cls == "TY1":
        return 1, s + 4, SGM_SGBM
    assert cls == "one_band"
    return nr + 4, nr + 4, SGM_HH4


def bands_of(c, mode=None, ty=None):
    """The main row bands of a one-pass launch of c under band height ty, as the kernel derives
    them: [(ty0, ty1, trips, tail, classes)] -- trips and tail of the row loop unrolled by U = 2 NR
    (None for a block that returns before its first barrier)."""
    mode = c.mode if mode is None else mode
    ty = c.ty if ty is None else ty
    H, s, nr = c.H, c.bs // 2, c.bs
    U, ylim, hh = 2 * nr, max(H - 1 - s, 0), is_hh(mode)
    nb = (H + ty - 1) // ty
    out = []
    for by in range(nb):
        ty0, ty1 = by * ty, min(by * ty + ty, H)
        yl = max(ty0, min(ty1, max(1, H - s))) if hh else ty1
        cls = set()
        if ty == 1:
            cls.add("TY1")
        if nb == 1:
            cls.add("one_band")
        if nb > 1 and by == nb - 1 and ty1 - ty0 < ty:
            cls.add("short_last")
        if yl <= ty0:
            out.append((ty0, ty1, None, None, cls | {"hh_p2_only"}))
            continue
        if hh and ty0 < yl < ty1:
            cls.add("hh_straddles_yl")
        if not hh and ty0 > ylim:
            cls.add("frozen")
        if not hh and ty0 <= ylim < ty1 - 1:
            cls.add("straddles_ylim")
        tfirst, tlast = min(ty0, ylim), min(yl - 1, ylim)
        n = tlast - tfirst + 1 + 2 * s
        trips, tail = n // U, n % U
        cls.add("n<U" if trips == 0 else "n>=3U" if trips >= 3 else
                "n==U" if (trips, tail) == (1, 0) else "n==U+1" if (trips, tail) == (1, 1) else
                "n==3U-1" if (trips, tail) == (2, U - 1) else "other")
        out.append((ty0, ty1, trips, tail, cls))
    return out


BAND_KERNELS = [(5, 1), (5, 2), (7, 1), (7, 2), (11, 1), (11, 2)]


def _band(cls, nr, k):
    ty, H, mode = band_shape(cls, nr)
    c = _cost(f"band_{cls}__k_{nr}_{k}", nr, 16 if k == 1 else 144, 37 if k == 1 else 21, H, mode)
    c.ty, c.cls = ty, cls
    return c


BAND_CASES = [_band(cls, nr, k) for nr, k in BAND_KERNELS for cls in BAND_CLASSES]


# ---- end to end ---------------------------------------------------------------------------

def random_cases(n, seed):
    """n seeded cases over the whole parameter domain of the census cost (numpy's generator: the
    survey never depends on an optional package)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        mode = int(rng.integers(0, 4))
        bs = int(rng.choice(BLOCK_SIZES))
        D = 16 * int(rng.integers(1, 17))
        minD = int(rng.integers(-40, 9))
        H = int(rng.integers(4, 37))
        W1 = int(rng.integers(bs // 2 + 1, 121))
        W = width_of(W1, minD, D)
        pmax = p2_census_max(bs)
        P1 = int(rng.integers(1, min(pmax - 1, 2000) + 1))
        P2 = pmax if rng.integers(0, 2) else int(rng.integers(P1 + 1, pmax + 1))
        kinds = [k for k in KINDS if k != "ramps" or W <= 256]
        out.append(SimpleNamespace(
            mode=mode, bs=bs, D=D, minD=minD, H=H, W1=W1, W=W, P1=P1, P2=P2,
            uniq=int(rng.choice([0, 1, 10, 15, 50])), uniq_rule=int(rng.integers(0, 3)),
            nstripes=int(rng.choice([1, 2, 3, 4, 8])), d12=int(rng.choice([1, 2, 1000000])),
            speckle=(0, 0) if rng.integers(0, 2) else (int(rng.choice([10, 100])), int(rng.integers(1, 5))),
            kind=str(rng.choice(kinds)), seed=int(rng.integers(0, 10**6)), index=i))
    return out


def random_args(c):
    return (c.minD, c.D, c.bs, c.P1, c.P2, c.d12, 0, c.uniq, c.speckle[0], c.speckle[1], c.mode)


def sgm_of(L, R, args, stages=3, **kw):
    """The pin's map under StereoSGBM.create's positional arguments."""
    minD, D, bs, P1, P2, d12, _, uniq, ws, sr, mode = args
    return CR.sgm_census(L, R, minD, D, bs, P1, P2, d12, uniq, ws, sr, mode, stages=stages, **kw)
