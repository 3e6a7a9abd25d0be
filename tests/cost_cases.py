"""Shapes, inputs and references shared by the Birchfield-Tomasi cost edge tests
(test_gpu_cost_edges.py) and the CPU check that they reach what they claim
(test_cost_cases_cpu.py).  Nothing here needs a GPU.

The BT cost has three kernels (csrc/sdr_cost.hip, sdr_cost_kernel.hpp, sdr_cost_generic.hip).
k_prefilter stages a row and its neighbours four bytes a lane when the row bytes W * cn, both
strides and the base are multiples of 4, a byte a lane otherwise, and walks the row 256 columns a
trip.  k_cost<NR, K, CN> has 22 reachable instantiations: NR = blockSize in {1, 3, 5, 7, 9, 11},
K = 1 (D <= 128, column blocks of BCOLS = 32) or 2 (D > 128, BCOLS = 16), CN = 1 or 3 -- blockSize 11
with three channels is outside the int16 cost domain at every preFilterCap, so the plan refuses it.
A block owns a band of TY rows and walks n = tlast - tfirst + 1 + 2 SH2 virtual rows in a loop
unrolled by U = 2 NR: n // U full trips, then a tail of n % U rows.  The launcher's own TY is the
tallest band that fills the device in one pass and at least 4, which on a small frame is always 4:
the band entries set TY through the debug knob SDR_DEBUG_COST_ROWS instead.  blockSize 13..17 or
D > 256 takes the two-pass generic cost: k_hsum_generic in strips of 64 columns, k_vsum_generic in
chunks of 32 rows.  The tables below name what each entry reaches.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import census_cases as CC
import numpy_ref as N
from census_cases import (BAND_CLASSES, BAND_CLASSES_BS1, band_shape, bands_of, bcols_of, is_hh, transform_layout,
                          width_of)
from numpy_ref import SGM_3WAY, SGM_HH, SGM_HH4, SGM_SGBM
from test_plan_cpu import stripes_of

BLOCK_SIZES = (1, 3, 5, 7, 9, 11)
MODES = (SGM_SGBM, SGM_HH, SGM_3WAY, SGM_HH4)
KINDS = ("noise", "binary", "ties", "flat", "steps", "periodic", "const")
CAPS = (15, 63, 127, 128, 255, 1000)
# every k_cost<NR, K, CN> the ABI reaches
INSTANTIATIONS = [(nr, k, 1) for k in (1, 2) for nr in BLOCK_SIZES] + \
                 [(nr, k, 3) for k in (1, 2) for nr in BLOCK_SIZES if nr < 11]
HSUM_STRIP, VSUM_CHUNK = 64, 32   # kHsumStrip, kVsumChunk


def ftzero_of(cap):
    return max(cap, 15) | 1


def p2_max(bs, cap, cn=1):
    """The largest P2 of the BT cost domain, 2*P2 + cn*(min(2*ftzero, 255) + 63)*blockSize^2 <= 32767
    (negative: the block term alone leaves the domain)."""
    return (32767 - cn * (min(2 * ftzero_of(cap), 255) + 63) * bs * bs) // 2


def other_hh_mode(mode):
    """A mode of the other hh_bottom class."""
    return SGM_3WAY if is_hh(mode) else SGM_HH


def kernel_of(bs, D, cn=1):
    """("k_cost", NR, K, CN) of the instantiation a call takes, ("generic", 0, 0, CN) past it."""
    if bs > 11 or D > 256:
        return ("generic", 0, 0, cn)
    return ("k_cost", bs, 1 if D <= 128 else 2, cn)


# ---- inputs -------------------------------------------------------------------------------

def _gray_pair(kind, H, W, D, seed):
    if kind == "ties":
        return CC.ties_pair(H, W, seed)
    if kind == "const":
        rng = np.random.default_rng(seed)
        a, b = (int(v) for v in rng.choice(256, 2, replace=False))
        return np.full((H, W), a, np.uint8), np.full((H, W), b, np.uint8)
    return CC.S.adversarial_pair(kind, H, W, D, seed=seed)


@lru_cache(maxsize=None)
def pair(kind, H, W, D=16, seed=0, cn=1):
    """The input pair of a case (read-only, computed once).  A colour frame has three independently
    drawn channels, so an L channel paired with the wrong R channel shows."""
    if cn == 1:
        L, R = _gray_pair(kind, H, W, D, seed)
    else:
        ch = [_gray_pair(kind, H, W, D, seed + 7919 * (c + 1)) for c in range(cn)]
        L, R = np.stack([p[0] for p in ch], -1), np.stack([p[1] for p in ch], -1)
    L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


def const_levels(L, R):
    """(a, b) per channel of a constant pair."""
    return [(int(l), int(r)) for l, r in zip(np.atleast_1d(L[0, 0]), np.atleast_1d(R[0, 0]))]


# ---- the references -----------------------------------------------------------------------

def pin_volume(L, R, minD, D, bs, P2, cap, mode):
    """The pin of stage 0, [H][W1][D] int16: numpy_ref.cost_volume (prefilter_channels, envelope,
    bt_cost_volume_rows and the box with OpenCV's border rules)."""
    return N.cost_volume(L, R, minD, D, bs, P2, ftzero_of(cap), hh=is_hh(mode))


def operand_planes(img, ftzero):
    """[cn][6][H][W] int: per channel the Sobel value, its lo and hi, the raw value, its lo and hi
    (lo / hi: numpy_ref.envelope over the value and its two half-sample neighbours)."""
    chans = [img] if img.ndim == 2 else [img[:, :, c] for c in range(img.shape[2])]
    out = []
    for ch in chans:
        sob, raw = N.prefilter_channels(ch, ftzero)
        out.append(np.stack([sob, *N.envelope(sob), raw, *N.envelope(raw)]))
    return np.stack(out)


def operand_planes_loop(img, ftzero):
    """operand_planes as a plain loop over pixels, every border rule spelled out.  Tiny images."""
    I = np.asarray(img).astype(int)
    if I.ndim == 2:
        I = I[:, :, None]
    H, W, cn = I.shape
    out = np.zeros((cn, 6, H, W), np.int64)

    def value(c, y, x):
        if x <= 0 or x >= W - 1:
            return ftzero & 0xff, ftzero & 0xff
        g = 0
        for dy, w in ((-1, 1), (0, 2), (1, 1)):
            yy = min(max(y + dy, 0), H - 1)
            g += w * (I[yy, x + 1, c] - I[yy, x - 1, c])
        return (min(max(g, -ftzero), ftzero) + ftzero) & 0xff, I[y, x, c]

    for c in range(cn):
        for y in range(H):
            for x in range(W):
                here = value(c, y, x)
                for k in range(2):
                    v = here[k]
                    a = (v + value(c, y, x + 1)[k]) >> 1 if x < W - 1 else v
                    b = (v + value(c, y, x - 1)[k]) >> 1 if x > 0 else v
                    out[c, 3 * k:3 * k + 3, y, x] = v, min(a, b, v), max(a, b, v)
    return out


def stage8_pin(img, ftzero):
    """Stage 8 of one frame's left-role image, [H][W][3cn] u32: per channel {sob | sob_lo << 16}
    {sob_hi | raw << 16} {raw_lo | raw_hi << 16}."""
    p = operand_planes(img, ftzero).astype(np.uint32)          # [cn][6][H][W]
    words = p[:, 0::2] | (p[:, 1::2] << np.uint32(16))         # [cn][3][H][W]
    return np.ascontiguousarray(words.reshape(-1, *words.shape[2:]).transpose(1, 2, 0))


def stage9_pin(img, ftzero):
    """Stage 9 of one frame's right-role image, [3cn][H][W] u64: q(x) | q(max(x-1, 0)) << 16 with
    q = {sob | sob_lo << 32} {sob_hi | raw << 32} {raw_lo | raw_hi << 32}."""
    p = operand_planes(img, ftzero).astype(np.uint64)
    q = p[:, 0::2] | (p[:, 1::2] << np.uint64(32))             # [cn][3][H][W]
    q = q.reshape(-1, *q.shape[2:])
    prev = np.concatenate([q[:, :, :1], q[:, :, :-1]], 2)
    return q | (prev << np.uint64(16))


def stage9_loop(img, ftzero):
    p = operand_planes_loop(img, ftzero)
    cn, _, H, W = p.shape
    out = np.zeros((3 * cn, H, W), np.uint64)
    for c in range(cn):
        for k in range(3):
            for y in range(H):
                for x in range(W):
                    xp = max(x - 1, 0)
                    q, qp = (int(p[c, 2 * k, y, xx]) | int(p[c, 2 * k + 1, y, xx]) << 32 for xx in (x, xp))
                    out[3 * c + k, y, x] = q | qp << 16
    return out


def const_closed_form(levels, H, W, minD, D, bs, P2, mode):
    """(value, mask [H][W1][D]) of a constant pair's volume, from the definition alone: away from
    the border columns every Sobel value is ftzero on both sides (cost 0) and every raw envelope is
    the level itself, so a channel's pixel cost is |a - b| >> 2, and C == P2 + sum over channels of
    bs^2 * (|a - b| >> 2) on every cell whose box keeps x and x - d inside columns 2..W-3 (columns
    1 and W-2 hold the level too, but their half-sample envelope reaches the border column's
    ftzero, which can lower the cost).  The rows are identical, so no vertical rule matters;
    MODE_HH's frozen rows hold P2 (second mask)."""
    maxD = minD + D
    minX1, W1 = max(maxD, 0), W + min(minD, 0) - max(maxD, 0)
    s = bs // 2
    x = minX1 + np.arange(W1)[:, None]
    d = minD + np.arange(D)[None, :]
    inner = (x >= 2) & (x <= W - 3) & (x - d >= 2) & (x - d <= W - 3)
    xi = np.clip(np.arange(W1)[:, None] + np.arange(-s, s + 1)[None, :], 0, W1 - 1)
    mask = np.broadcast_to(inner[xi].all(1), (H, W1, D)).copy()
    frozen = np.zeros((H, W1, D), bool)
    if is_hh(mode):
        frozen[max(1, H - s):] = True
        mask &= ~frozen
    return P2 + bs * bs * sum(abs(a - b) >> 2 for a, b in levels), mask, frozen


# ---- the table ----------------------------------------------------------------------------

def _case(name, bs, D, W1, H, mode, minD=0, kind="noise", P2=None, F=1, cn=1, cap=15, ty=0, ns=4, tags=()):
    W = width_of(W1, minD, D)
    pmax = p2_max(bs, cap, cn)
    if P2 is None:
        P2 = min(12 * bs * bs, pmax)
    elif P2 == "max":
        P2 = pmax
    return SimpleNamespace(name=name, id=name, bs=bs, D=D, W1=W1, H=H, W=W, mode=mode, minD=minD, kind=kind,
                           P1=min(2 * bs * bs, P2 - 1), P2=P2, F=F, cn=cn, cap=cap, ty=ty, ns=ns, tags=tuple(tags))


W1_CLASSES = ("sw2+1", "bcols-1", "bcols", "bcols+1", "3bcols+5")
D_CLASSES = {1: (16, 64, 128), 2: (144, 256)}
H_CLASSES = ("1", "sh2", "sh2+1", "2sh2+1", "2sh2+2")


def w1_of(cls, bs, D):
    b, s = bcols_of(D), bs // 2
    return {"sw2+1": s + 1, "bcols-1": b - 1, "bcols": b, "bcols+1": b + 1, "3bcols+5": 3 * b + 5}[cls]


def w1_class(c):
    return {w1_of(k, c.bs, c.D): k for k in W1_CLASSES}.get(c.W1)


def h_of(cls, bs):
    s = bs // 2
    return {"1": 1, "sh2": s, "sh2+1": s + 1, "2sh2+1": 2 * s + 1, "2sh2+2": 2 * s + 2}[cls]


def _instantiation_cases():
    """Every reachable <NR, K, CN>, the W1 classes, the D classes of each K, the modes and three
    input kinds dealt round over them.  Colour K = 2 at D = 256 asks for more than 64 KiB of LDS
    from NR = 3 on."""
    out = []
    for i, (nr, k, cn) in enumerate(INSTANTIATIONS):
        cls = W1_CLASSES[(i + i // 5) % 5]
        D = D_CLASSES[k][(i + (cn == 3)) % len(D_CLASSES[k])]
        out.append(_case(f"k_{nr}_{k}_{cn}__W1_{cls}__D{D}", nr, D, w1_of(cls, nr, D), nr + 5 + i % 4, MODES[i % 4],
                         kind=("noise", "binary", "ties")[i % 3], cn=cn, P2="max" if i % 2 else None,
                         tags=("instantiation",)))
    # colour K = 2 at the widest range of every NR: the largest dynamic LDS requests
    for nr in (3, 5, 7, 9):
        out.append(_case(f"k_{nr}_2_3__D256_lds", nr, 256, 21, nr + 6, MODES[nr // 2 % 4], cn=3, tags=("lds",)))
    return out


BAND_KERNELS = [(nr, 1) for nr in BLOCK_SIZES] + [(5, 2), (11, 2)]


def _band_cases():
    out = []
    for nr, k in BAND_KERNELS:
        D, W1 = (16, 37) if k == 1 else (144, 21)
        for cls in (BAND_CLASSES_BS1 if nr == 1 else BAND_CLASSES):
            ty, H, mode = band_shape(cls, nr)
            out.append(_case(f"band_{cls}__k_{nr}_{k}", nr, D, W1, H, mode, ty=ty, tags=("band", cls)))
    # three channels through the steady-state loop too
    out.append(_case("band_n>=3U__k_9_1_3", 9, 16, 37, 60, SGM_SGBM, ty=48, cn=3, tags=("band", "n>=3U")))
    return out


def _edge_cases():
    out = []
    # frame heights around the vertical window, blockSize 7 (SH2 = 3) and 11 (SH2 = 5)
    for bs in (7, 11):
        for i, cls in enumerate(H_CLASSES):
            D, W1 = ((16, 40), (144, 20), (64, 37))[i % 3]
            out.append(_case(f"H_{cls}__bs{bs}", bs, D, W1, h_of(cls, bs), MODES[(i + bs) % 4],
                             kind=("noise", "ties")[i % 2], cn=3 if (bs, cls) == (7, "2sh2+1") else 1, tags=("height", cls)))
    # the disparity range's position: the staging clamp min(max(xr0 + ir, 0), W - 1) and gl's clamp
    out += [
        _case("minD_3", 5, 64, 40, 14, SGM_SGBM, minD=3, tags=("minD",)),
        _case("minD_-20__k2", 3, 144, 20, 9, SGM_3WAY, minD=-20, kind="ties", tags=("minD",)),
        _case("minD_-20__k1", 9, 16, 37, 13, SGM_HH, minD=-20, tags=("minD",)),
        _case("minD_-20__k1_cn3", 5, 16, 33, 9, SGM_SGBM, minD=-20, cn=3, tags=("minD",)),
        _case("maxD_negative", 5, 16, 45, 12, SGM_SGBM, minD=-40, tags=("minD",)),
        _case("maxD_negative__k2", 3, 144, 21, 7, SGM_HH4, minD=-200, kind="ties", tags=("minD",)),
    ]
    # preFilterCap: the clip table's and tab[0]'s & 0xff wraps, the int16 domain met at its edge
    for i, cap in enumerate(CAPS):
        cn = 3 if i % 2 else 1
        bs = 3 if cn == 3 else 5
        out.append(_case(f"cap_{cap}__cn{cn}_P2max", bs, (16, 144)[i // 3 % 2], 37, 11, MODES[i % 4], kind="binary",
                         P2="max", cn=cn, cap=cap, tags=("cap",)))
    # input kinds, gray and colour
    for i, kind in enumerate(KINDS):
        for cn in (1, 3):
            out.append(_case(f"kind_{kind}__cn{cn}", (5, 3, 7)[i % 3], (64, 144)[(i + cn) % 2], 38, 10,
                             MODES[(i + cn) % 4], kind=kind, cn=cn, tags=("kind",)))
    out.append(_case("const__bs11_hh", 11, 16, 50, 14, SGM_HH, kind="const", P2="max", tags=("kind",)))
    # batches: every frame is compared
    for k, D in ((1, 64), (2, 144)):
        for cn in (1, 3):
            out.append(_case(f"batch3__k{k}_cn{cn}", (5, 7)[k - 1], D, 37, 11, (SGM_3WAY, SGM_HH)[k - 1],
                             kind=("noise", "ties")[k - 1], F=3, cn=cn, tags=("batch",)))
    return out


def _generic_cases():
    """The two-pass cost: blockSize 13..17 (gray, cap 15: the colour block term leaves the domain) or
    D > 256.  H classes around kVsumChunk = 32 rows, W1 classes around kHsumStrip = 64 columns."""
    g = ("generic",)
    return [
        _case("generic_bs13__W1_63__H31", 13, 16, 63, 31, SGM_SGBM, P2="max", kind="binary", tags=g),
        _case("generic_bs15__W1_64__H32", 15, 32, 64, 32, SGM_3WAY, tags=g),
        _case("generic_bs17__W1_65__H33", 17, 16, 65, 33, SGM_HH, P2="max", tags=g),
        _case("generic_bs13__W1_129__H65", 13, 16, 129, 65, SGM_HH4, kind="ties", tags=g),
        # MODE_HH's first P2 row, H - SH2 = 32, starts a chunk
        _case("generic_bs13__hh_yl_on_chunk", 13, 16, 40, 38, SGM_HH, tags=g + ("yl_on_chunk",)),
        _case("generic_bs15__D48_24pairs", 15, 48, 66, 20, SGM_SGBM, tags=g + ("D48",)),
        _case("generic_D272", 5, 272, 30, 12, SGM_SGBM, kind="ties", tags=g),
        _case("generic_D320__cn3", 3, 320, 20, 9, SGM_HH, cn=3, tags=g),
        _case("generic_D512", 9, 512, 17, 13, SGM_3WAY, tags=g),
        _case("generic_D272__cn3__W1_65", 7, 272, 65, 10, SGM_HH4, cn=3, P2="max", kind="binary", tags=g),
        _case("generic_D512__cn3", 1, 512, 9, 7, SGM_SGBM, cn=3, tags=g),
        _case("generic_D320__bs11_minD-20", 11, 320, 25, 15, SGM_HH, minD=-20, tags=g),
        _case("generic_batch3__bs13", 13, 16, 70, 34, SGM_HH, F=3, tags=g + ("batch",)),
        _case("generic_batch3__D272_cn3", 3, 272, 20, 8, SGM_3WAY, F=3, cn=3, tags=g + ("batch",)),
    ]


COST_CASES = _instantiation_cases() + _band_cases() + _edge_cases() + _generic_cases()
COST_BY_ID = {c.id: c for c in COST_CASES}
BAND_CASES = [c for c in COST_CASES if "band" in c.tags]


def cost_pairs(c):
    """The F input pairs of a cost case."""
    return [pair(c.kind, c.H, c.W, c.D, seed=2000 + 7 * f + len(c.name), cn=c.cn) for f in range(c.F)]


def create_args(c, mode=None, uniq=12, d12=1):
    """StereoSGBM.create's positional arguments of a case."""
    return (c.minD, c.D, c.bs, c.P1, c.P2, d12, c.cap, uniq, 0, 0, c.mode if mode is None else mode)


@lru_cache(maxsize=None)
def _pin_cached(cid, f, hh):
    c = COST_BY_ID[cid]
    L, R = cost_pairs(c)[f]
    out = pin_volume(L, R, c.minD, c.D, c.bs, c.P2, c.cap, SGM_HH if hh else SGM_SGBM)
    out.setflags(write=False)
    return out


def pin_of(c, f, mode):
    """The pin of frame f of a table entry under a mode (computed once, read-only)."""
    return _pin_cached(c.id, f, is_hh(mode))


# ---- MODE_SGBM_3WAY stripes ---------------------------------------------------------------

def _stripe(H, W, D, bs, ns, kind="noise", cn=1):
    c = _case(f"stripes_{H}x{W}_d{D}_bs{bs}_ns{ns}_{kind}_cn{cn}", bs, D, W - D, H, SGM_3WAY, kind=kind, cn=cn, ns=ns,
              tags=("stripes",))
    return c


STRIPE_CASES = [
    # every row of the last stripes keeps its window clamped at the stripe start (aux_rows == end - s0)
    *[_stripe(H, 70, 32, bs, ns) for bs, H, ns in ((7, 15, 8), (9, 14, 4), (9, 17, 8), (9, 26, 8), (11, 15, 8),
                                                    (11, 18, 4), (11, 21, 8))],
    _stripe(31, 60, 16, 5, 1, "ties"),        # one stripe: the frame, no band
    _stripe(31, 60, 16, 5, 3, "noise"),
    _stripe(31, 60, 16, 5, 4, "ties", cn=3),  # SH2 rows a band, colour
    _stripe(31, 60, 16, 5, 8, "binary"),
    _stripe(33, 180, 144, 3, 3, "noise"),     # K = 2
    _stripe(26, 170, 144, 9, 8, "ties"),      # K = 2, short last stripes
    _stripe(21, 165, 144, 7, 4, "noise", cn=3),  # K = 2, colour, short last stripes
    _stripe(9, 60, 16, 1, 4, "noise"),        # blockSize 1: SH2 = 0, no band holds a row
    _stripe(9, 60, 16, 1, 4, "noise", cn=3),
    _stripe(40, 56, 16, 13, 4, "noise"),      # the generic path's stripe bands
    _stripe(18, 300, 272, 5, 4, "ties"),
]


def stripe_pair(c):
    return pair(c.kind, c.H, c.W, c.D, seed=c.H, cn=c.cn)


def horizontal_sums(L, R, minD, D, bs, ftzero):
    """hs [H][W1][D]: the pixel cost summed over the box's columns, clamped to the matched ones."""
    pix = N.bt_cost_volume_rows(L, R, minD, D, ftzero).astype(np.int64)
    W1, s = pix.shape[1], bs // 2
    xi = np.clip(np.arange(W1)[:, None] + np.arange(-s, s + 1)[None, :], 0, W1 - 1)
    return pix[:, xi, :].sum(2)


def stripe_rows_ref(L, R, c, box=N._box_rows):
    """Stage 6's defined rows as [(stripe, rows [aux_rows][W1][D])] for the stripes that keep rows
    of their own, and the buffer's (stripes, rows a band) -- census_cases.stripe_rows_ref for the
    BT cost."""
    H, SH2 = c.H, c.bs // 2
    st = stripes_of(H, c.ns, c.bs, SH2)
    hs = horizontal_sums(L, R, c.minD, c.D, c.bs, ftzero_of(c.cap))
    out = [(s, c.P2 + box(hs, s0, s0 + aux, SH2, False)) for s, (s0, end, out0, aux) in enumerate(st) if aux]
    return out, (len(st), max(x[3] for x in st))


# ---- the prefilter ------------------------------------------------------------------------
# (name, H, W, cn, layout, cap): the matcher runs D = 16, blockSize 1, so W1 = W - 16 >= 1 at every
# width.  Layouts as census_cases.transform_layout's, in bytes of a row of W * cn.
PREFILTER_SHAPES = [
    # W * cn % 4 == 0, dense: the dword staging
    ("dword_20x3", 3, 20, 1, "dense", 15),
    ("dword_256x1_one_trip", 1, 256, 1, "dense", 63),
    ("dword_260x8_second_trip", 8, 260, 1, "dense", 127),
    ("dword_1024x2_four_trips", 2, 1024, 1, "dense", 128),
    ("dword_cn3_20x8", 8, 20, 3, "dense", 255),
    ("dword_cn3_256x2", 2, 256, 3, "dense", 1000),
    # the byte staging, reached by odd row bytes
    ("odd_17x1", 1, 17, 1, "dense", 1000),
    ("odd_255x2", 2, 255, 1, "dense", 255),
    ("odd_257x3_second_trip", 3, 257, 1, "dense", 128),
    ("odd_cn3_17x3", 3, 17, 3, "dense", 127),
    ("odd_cn3_85x1", 1, 85, 3, "dense", 63),
    ("odd_cn3_86x2", 2, 86, 3, "dense", 15),
    # ... by a row stride that is no multiple of 4 on aligned row bytes
    ("stride1_20x2", 2, 20, 1, ("stride", 1), 63),
    ("stride7_260x3", 3, 260, 1, ("stride", 7), 15),
    ("stride1_cn3_256x1", 1, 256, 3, ("stride", 1), 128),
    ("stride7_cn3_20x8", 8, 20, 3, ("stride", 7), 255),
    # ... by a misaligned base on aligned row bytes and stride
    ("base1_20x8", 8, 20, 1, "base1", 127),
    ("base1_256x3", 3, 256, 1, "base1", 1000),
    ("base1_cn3_20x2", 2, 20, 3, "base1", 15),
    # three frames whose frame stride is no multiple of 4 (aligned row bytes), aligned, and dense odd
    ("batch_20x3_fstride61", 3, 20, 1, ("batch", 1), 255),
    ("batch_cn3_20x2_fstride123", 2, 20, 3, ("batch", 3), 63),
    ("batch_260x2_aligned", 2, 260, 1, ("batch", 4), 128),
    ("batch_17x3_dense", 3, 17, 1, ("batch", 0), 127),
]
PREFILTER_KINDS = ("noise", "binary", "flat", "ties")
PREFILTER_WIDTHS = {1: {17, 20, 255, 256, 257, 260, 1024}, 3: {20, 17, 256, 85, 86}}
PREFILTER_HEIGHTS = {1, 2, 3, 8}


def takes_dword_path(W, cn, stride, fstride, base_mod4):
    """k_prefilter's own condition for the four-bytes-a-lane staging."""
    return ((W * cn | stride | fstride | base_mod4) & 3) == 0


def prefilter_frames(kind, H, W, cn, F):
    frames = [pair(kind, H, W, 16, seed=31 * f + W + H, cn=cn) for f in range(F)]
    return np.stack([p[0] for p in frames]), np.stack([p[1] for p in frames])
