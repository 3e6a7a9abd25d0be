"""Clouds, voxel-grid leaves and display frames shared by the emit edge tests
(test_gpu_cloud_edges.py, test_gpu_display_edges.py) and the CPU check that every case has the
property it is named for (test_emit_cases_cpu.py).  Every case is built from a seed on the CPU;
nothing here needs a GPU or imports the engine.  The threshold tables are found with the oracle
(a CPU library), which the callers pass in.

Voxel grid (sdr_cloud.hip): `lattice` clouds sit at known cells of a known grid, so the product of
the three divisions -- which sets the radix sort's pass count and marks the non-finite points --
lands on and next to 2^8, 2^16 and 2^24; sizes on and next to a block (256), a scan segment (2048)
and a sort tile (4096); anisotropic leaves; cell indices past 2^24; voxels of 70 000 points;
PCL's passthrough decision on either side of 2^31.

Display (sdr_display.hip): for each of the 255 output levels of the gamma map and of the depth map,
the first float that reaches it (found by bisection over float bit patterns) with its neighbours;
frames that hold all 65 536 operand pairs of each addWeighted; the Z values on which k_zstats and
the range recurrence compare, at the lanes and columns where a wave or a block ends.
"""
import itertools
from types import SimpleNamespace

import numpy as np

SENT = 0xA5
LEAF = (0.5, 0.25, 2.0)
ORIGIN = (-37.0, 11.5, -1000.0)  # whole cells of LEAF: (-74, 46, -500)
NONFINITE = (np.nan, np.inf, -np.inf)
F32 = np.float32


def ro(a):
    a.setflags(write=False)
    return a


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- voxel grid: numpy restatement ---------------------------------------------------------------

def voxel_params(pts, leaf):
    """What pcl::VoxelGrid derives from the finite points, float32 as PCL: inv, mn, mx, d (the int64
    extents of the overflow check), prod (their product, wrapped like compiled code), minb, div,
    past (the product of div).  None without a finite point."""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 4)
    inv = F32(1.0) / np.asarray(leaf, F32)
    fin = np.isfinite(pts[:, :3]).all(1)
    if not fin.any():
        return None
    q = pts[fin, :3]
    mn, mx = q.min(0), q.max(0)
    d = [int(v) + 1 for v in ((mx - mn) * inv).astype(np.int64)]
    prod = (d[0] * d[1] * d[2]) & (2**64 - 1)
    prod = prod - 2**64 if prod >= 2**63 else prod
    fmin = np.floor(mn * inv)
    minb = fmin.astype(np.int64)
    div = np.floor(mx * inv).astype(np.int64) - minb + 1
    return SimpleNamespace(inv=inv, fin=fin, mn=mn, mx=mx, d=d, prod=prod, fmin=fmin, minb=minb, div=div,
                           past=int(div[0]) * int(div[1]) * int(div[2]))


def np_voxel(pts, leaf, int_minb=False):
    """pcl::VoxelGrid<PointXYZRGB> in numpy, any leaf: float32 throughout, a stable sort of the
    voxel index, in-voxel sums sequential in point order -> (points (M, 4), passthrough).
    int_minb subtracts min_b after the cast to int instead of before it, in float."""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 4)
    P = voxel_params(pts, leaf)
    if P is None:
        return np.empty((0, 4), F32), False
    if P.prod > 2**31 - 1:
        return pts.copy(), True
    q = pts[P.fin]
    fl = np.floor(q[:, :3] * P.inv)
    ijk = fl.astype(np.int64) - P.minb if int_minb else (fl - P.minb.astype(F32)).astype(np.int64)
    mul1, mul2 = int(P.div[0]) & 0xFFFFFFFF, (int(P.div[0]) * int(P.div[1])) & 0xFFFFFFFF
    idx = (ijk[:, 0] + ijk[:, 1] * mul1 + ijk[:, 2] * mul2) & 0xFFFFFFFF
    order = np.argsort(idx, kind="stable")
    sidx, sq = idx[order], q[order]
    c = sq.view(np.uint32)[:, 3]
    vals = np.stack([sq[:, 0], sq[:, 1], sq[:, 2], ((c >> 16) & 255).astype(F32), ((c >> 8) & 255).astype(F32),
                     (c & 255).astype(F32), (c >> 24).astype(F32)], 1).astype(F32)
    starts = np.flatnonzero(np.r_[True, sidx[1:] != sidx[:-1]])
    ends = np.r_[starts[1:], len(sidx)]
    out = np.empty((len(starts), 4), F32)
    zero = np.zeros((1, 7), F32)  # the sums start at +0: a voxel of -0.0 alone has the centroid +0.0
    for k, (a, b) in enumerate(zip(starts, ends)):
        m = np.cumsum(np.r_[zero, vals[a:b]], axis=0, dtype=F32)[-1] / F32(b - a)
        out[k, :3] = m[:3]
        out.view(np.uint32)[k, 3] = int(m[6]) << 24 | int(m[3]) << 16 | int(m[4]) << 8 | int(m[5])
    return out, False


# ---- voxel grid: clouds ----------------------------------------------------------------------------

def random_rgba(rng, n, lo=0):
    b = rng.integers(lo, 256, (n, 4), dtype=np.uint32)
    return b[:, 0] << 24 | b[:, 1] << 16 | b[:, 2] << 8 | b[:, 3]


def spoil(pts, idx):
    """Makes the points `idx` non-finite: NaN, +inf and -inf in x, y and z in turn."""
    for j, i in enumerate(idx):
        pts[i, j % 3] = NONFINITE[(j // 3) % 3]
    return pts


def lattice(dims, n, leaf=LEAF, origin=ORIGIN, seed=0, share=0.1):
    """n points at (ijk + U(0.25, 0.75)) * leaf + origin, ijk uniform in dims, random rgba over all
    32 bits; `share` of them non-finite, index 0 and index n - 1 among them.  The first finite
    point sits in cell (0, 0, 0) and the second in cell dims - 1, so the grid's divisions are dims
    whenever origin is a whole number of leaves; the middle and the last finite point sit in cell
    (0, 0, 0) as well."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, np.int64)
    ijk = rng.integers(0, dims, (n, 3))
    u = rng.uniform(0.25, 0.75, (n, 3))
    bad = np.zeros(n, bool)
    k = int(round(share * n))
    if k >= 2 and n >= 8:
        bad[[0, n - 1]] = True
        bad[rng.choice(np.arange(1, n - 1), k - 2, replace=False)] = True
    fin = np.flatnonzero(~bad)
    if len(fin) >= 1:
        ijk[fin[0]] = 0
    if len(fin) >= 2:
        ijk[fin[1]] = dims - 1
    if len(fin) >= 8:
        # cell 0 again in the middle and at the end, with non-finite points in between: should
        # those sort to voxel 0 instead of last, they cut its run in pieces
        ijk[fin[len(fin) // 2]] = ijk[fin[-1]] = 0
    pts = np.empty((n, 4), F32)
    pts[:, :3] = ((ijk + u) * np.asarray(leaf, np.float64) + np.asarray(origin, np.float64)).astype(F32)
    pts.view(np.uint32)[:, 3] = random_rgba(rng, n)
    return spoil(pts, np.flatnonzero(bad))


BAND_DIMS = [(15, 17, 1), (16, 16, 1), (255, 257, 1), (256, 256, 1), (255, 255, 258), (256, 256, 256),
             (2047, 1024, 1024)]
BAND_BITS = [8, 9, 16, 17, 24, 25, 31]  # bit length of the product: 1, 2, 2, 3, 3, 4, 4 sort passes
SIZES = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8193]
PERMS = sorted(set(itertools.permutations(LEAF)))
ISO = [(v, v, v) for v in LEAF]
LONG_N = 70000
EDGE_DIMS = (46341, 46340, 1)  # 46341 * 46340 = 2^31 - 1 - 41707; 46341^2 = 2^31 + 4633


def _one_finite(n, keep):
    pts = lattice((7, 5, 3), n, seed=300, share=0.0)
    return spoil(pts, [i for i in range(n) if i not in keep])


def _long_run(n, seed, singles=0):
    """n points inside one cell of a unit grid, colour bytes 248..255 so that 70 000 of them pass
    2^24; then `singles` points, one in each cell of a row next to it."""
    rng = np.random.default_rng(seed)
    pts = np.empty((n + singles, 4), F32)
    pts[:n, :3] = rng.uniform(0.05, 0.95, (n, 3)) + [3.0, -2.0, 7.0]
    pts[n:, :3] = rng.uniform(0.05, 0.95, (singles, 3)) + [3.0, -2.0, 7.0]
    pts[n:, 0] += np.arange(1, singles + 1)
    pts.view(np.uint32)[:, 3] = random_rgba(rng, n + singles, 248)
    return pts[rng.permutation(n + singles)] if singles else pts


def _edge(past):
    """Leaf 1: corner points 0.25 into cell 0 and 0.75 into cell dims - 1, so that PCL's extents
    (int64)((max - min) * inv) + 1 are EDGE_DIMS exactly; with `past` the far corner sits one cell
    further in y, which is all that differs between the two clouds."""
    pts = lattice(EDGE_DIMS, 4097, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 46341)
    fin = np.flatnonzero(np.isfinite(pts[:, :3]).all(1))
    pts[fin[0], :3] = 0.25
    pts[fin[1], :3] = np.asarray(EDGE_DIMS, np.float64) - 0.25
    if past:
        pts[fin[1], 1] += 1.0
    return pts


def _ties():
    """Points exactly on cell boundaries of a 0.5 grid (k * 0.5, k of either sign), -0.0 and +0.0."""
    rng = np.random.default_rng(77)
    k = rng.integers(-6, 7, (600, 3))
    pts = np.empty((600, 4), F32)
    pts[:, :3] = k * 0.5
    pts[::7, 0] = -0.0
    pts[3::7, 1] = 0.0
    pts[5::11, 2] = -0.0
    pts.view(np.uint32)[:, 3] = random_rgba(rng, 600)
    return pts


WIDE_FAR = (33554424.0, 33554426.0, 33554428.0, 33554430.0, 33554432.0, 33554436.0, 33554440.0)


def _wide_axis(near):
    """Leaf 1 and more than 2^24 cells along x: 200 points in the odd cell `near`, 400 in the seven
    cells WIDE_FAR on either side of 2^25 (each a float).  floorf(x) - (float)min_b is not a float
    for them, so PCL's float subtraction rounds and merges cells that an integer subtraction after
    the cast keeps apart."""
    rng = np.random.default_rng(25)
    pts = np.empty((600, 4), F32)
    pts[:, :3] = rng.uniform(0.1, 0.9, (600, 3))
    pts[:200, 0] += near
    pts[200:, 0] = np.asarray(WIDE_FAR, F32)[rng.integers(0, len(WIDE_FAR), 400)]
    pts[200:207, 0] = WIDE_FAR
    pts.view(np.uint32)[:, 3] = random_rgba(rng, 600)
    return pts[rng.permutation(600)]


def _builders():
    b = {}
    for dims in BAND_DIMS:
        b["band-%dx%dx%d" % dims] = lambda dims=dims: (lattice(dims, 4097, seed=sum(dims)), LEAF)
    for n in SIZES:
        b[f"size-{n}"] = lambda n=n: (lattice((7, 5, 3), n, seed=n), LEAF)
    b["one-finite"] = lambda: (_one_finite(300, {137}), LEAF)
    b["none-finite"] = lambda: (_one_finite(300, set()), LEAF)
    for leaf in PERMS + ISO:
        b["aniso-%g-%g-%g" % leaf] = lambda leaf=leaf: (lattice((12, 20, 6), 4097, seed=5), leaf)
    # cell indices past 2^24 on one axis: floats there are 2 apart, so 5 cells fall into 3
    b["minb+x"] = lambda: (lattice((5, 5, 5), 1000, (0.001,) * 3, (20000.0, 0.1, -0.2), seed=9), (0.001,) * 3)
    b["minb-y"] = lambda: (lattice((5, 5, 5), 1000, (0.001,) * 3, (0.3, -20000.0, 0.1), seed=10), (0.001,) * 3)
    b["minb-wide+3"] = lambda: (_wide_axis(3.0), (1.0, 1.0, 1.0))
    b["minb-wide-5"] = lambda: (_wide_axis(-5.0), (1.0, 1.0, 1.0))
    b["long-one"] = lambda: (_long_run(LONG_N, 70), (1.0, 1.0, 1.0))
    b["long-mixed"] = lambda: (_long_run(20000, 71, 5000), (1.0, 1.0, 1.0))
    b["edge-below"] = lambda: (_edge(False), (1.0, 1.0, 1.0))
    b["edge-past"] = lambda: (_edge(True), (1.0, 1.0, 1.0))
    b["identical"] = lambda: (np.tile(lattice((1, 1, 1), 1, seed=3), (1000, 1)), LEAF)
    b["ties"] = lambda: (_ties(), (0.5, 0.5, 0.5))
    return b


_BUILD = _builders()
VOXEL_IDS = list(_BUILD)
_CLOUDS, _VREF = {}, {}


def voxel_case(cid):
    """(points (n, 4) float32, leaf) of a case, built once (read-only)."""
    if cid not in _CLOUDS:
        pts, leaf = _BUILD[cid]()
        _CLOUDS[cid] = (ro(np.ascontiguousarray(pts, F32)), tuple(float(v) for v in leaf))
    return _CLOUDS[cid]


def voxel_reference(oracle, cid):
    """oracle.voxel_grid of a case, computed once (read-only)."""
    if cid not in _VREF:
        pts, leaf = voxel_case(cid)
        out, passthrough = oracle.voxel_grid(pts, leaf)
        _VREF[cid] = (ro(out), passthrough)
    return _VREF[cid]


# ---- organised cloud -------------------------------------------------------------------------------

CLOUD_SHAPES = [(1, 1, 3), (255, 1, 3), (257, 1, 3), (37, 5, 3), (8192 * 256 + 1, 1, 1)]  # (W, H, F)


def cloud_frames(W, H, F, seed=0):
    """xyz (F, H, W, 3) with one pixel in sixteen non-finite, and BGR (F, H, W, 3) without SENT."""
    rng = np.random.default_rng(seed + W)
    xyz = rng.normal(0, 1000, (F, H, W, 3)).astype(F32)
    flat = xyz.reshape(-1, 3)
    bad = np.flatnonzero(rng.random(len(flat)) < 1 / 16)
    flat[bad, bad % 3] = np.asarray(NONFINITE, F32)[(bad // 3) % 3]
    flat[0, 0], flat[-1, 2] = np.nan, np.inf
    bgr = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    bgr[bgr == SENT] = SENT ^ 1
    return ro(xyz), ro(bgr)


def padded_u8(a, row_bytes, frame_bytes, fill=SENT):
    """(F, rows, n) uint8 laid out with rows row_bytes apart and frames frame_bytes apart in a flat
    buffer of `fill`."""
    F, R, n = a.shape
    buf = np.full(F * frame_bytes, fill, np.uint8)
    for f in range(F):
        for y in range(R):
            o = f * frame_bytes + y * row_bytes
            buf[o:o + n] = a[f, y]
    return buf


def padded_f32(a, stride, fstride, fill=np.nan):
    """(F, H, W) float32 with rows `stride` and frames `fstride` ELEMENTS apart, `fill` between."""
    F, H, W = a.shape
    buf = np.full(F * fstride, fill, F32)
    for f in range(F):
        for y in range(H):
            o = f * fstride + y * stride
            buf[o:o + W] = a[f, y]
    return buf


# ---- display: thresholds ---------------------------------------------------------------------------

NUM_DISP = (16, 80, 128, 256)
IDENT = ro(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1))  # a colour table that shows the level
ZR0 = (1000.0, 2000.0)
Z_LO, Z_HI = 500.0, 9000.0  # anchors: from ZR0 the range goes to exactly {950, 2700}
WIDE = 300
_TAB = {}


def bits(v):
    return int(np.asarray(v, F32).view(np.uint32))


def _bisect(level_of, lo, hi):
    """For want = 1..255 the smallest float bit pattern in (lo, hi] whose level is >= want;
    level_of maps 255 bit patterns to 255 levels, monotone, level(lo) = 0, level(hi) = 255."""
    want = np.arange(1, 256)
    lo, hi = np.full(255, lo, np.int64), np.full(255, hi, np.int64)
    calls = 0
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        ge = level_of(mid.astype(np.uint32)) >= want
        hi, lo = np.where(ge, mid, hi), np.where(ge, lo, mid)
        calls += 1
    return hi.astype(np.uint32), calls


def gamma_thresholds(oracle, nd):
    """t[v] for v = 1..255: the smallest disparity whose show_disparityMap level is >= v (t[0] = 0)."""
    if ("g", nd) not in _TAB:
        def level_of(b):
            return oracle.show_disparity_map(b.view(F32).reshape(1, -1), nd)[0]
        t, calls = _bisect(level_of, 0, bits(2.0 * nd))
        _TAB["g", nd] = (ro(np.r_[np.uint32(0), t].view(F32)), calls)
    return _TAB["g", nd][0]


def depth_levels(oracle, z, zr):
    """show_depthMap's levels of the values z in a frame that also holds the two anchors."""
    frame = np.r_[F32(Z_LO), F32(Z_HI), np.asarray(z, F32)].reshape(1, -1)
    return oracle.show_depth_map(frame, np.array(zr, np.float64), IDENT)[0, 2:, 0]


def range_after(zr, lo=Z_LO, hi=Z_HI):
    """The smoothed range one frame with raw minimum lo and maximum hi later (no clamp active)."""
    return (0.9 * zr[0] + 0.1 * lo, 0.9 * zr[1] + 0.1 * hi)


def depth_thresholds(oracle, zr=ZR0):
    """t[v] for v = 1..255: the smallest Z whose show_depthMap level is >= v, in a frame whose valid
    Z span the anchors, entered with the range state zr; t[0] = 600, a valid Z of level 0."""
    key = ("z",) + tuple(zr)
    if key not in _TAB:
        t, calls = _bisect(lambda b: depth_levels(oracle, b.view(F32), zr), bits(Z_LO), bits(Z_HI))
        _TAB[key] = (ro(np.r_[F32(600.0).view(np.uint32), t].view(F32)), calls)
    return _TAB[key][0]


def bisect_calls(key):
    return _TAB[key][1]


def _neighbours(t):
    """Each threshold of t[1:] with its 3 neighbours on either side, as float32 (255, 7)."""
    b = t[1:].view(np.uint32).astype(np.int64)[:, None] + np.arange(-3, 4)
    return b.astype(np.uint32).view(F32)


def _wide(vals, fill):
    h = -(-len(vals) // WIDE)
    out = np.full(h * WIDE, fill, F32)
    out[:len(vals)] = vals
    return ro(out.reshape(h, WIDE))


def gamma_specials(nd):
    return np.array([0.0, -0.0, 1e-45, nd, 2 * nd, np.inf, -np.inf, np.nan, -1.0], F32)


def gamma_frame(oracle, nd):
    """(H, 300): thresholds with neighbours (row-major, 7 a level), then gamma_specials, then -1."""
    return _wide(np.r_[_neighbours(gamma_thresholds(oracle, nd)).reshape(-1), gamma_specials(nd)], -1.0)


def depth_frame(oracle):
    """(H, 300): the two anchors, then thresholds with neighbours, then Z = 1000."""
    return _wide(np.r_[F32(Z_LO), F32(Z_HI), _neighbours(depth_thresholds(oracle)).reshape(-1)], 1000.0)


# ---- display: all operand pairs of addWeighted ------------------------------------------------------

def overlay_pairs():
    """vis (256, 256) with vis[y, x] = x and a left view (512, 512, 3) whose 2 x 2 blocks are
    constant y: with IDENT as the table, pixel (y, x) blends lc = y with hc = x."""
    vis = np.tile(np.arange(256, dtype=np.uint8), (256, 1))
    left = np.repeat(np.repeat(np.arange(256, dtype=np.uint8), 2)[:, None], 512, 1)
    return ro(vis), ro(np.ascontiguousarray(np.repeat(left[:, :, None], 3, 2)))


def ema_disp_frames(oracle, nd=80):
    """(2, 256, 256): frame 0 has level y, frame 1 level x, so the EMA sees (prev, new) = (y, x)."""
    t = gamma_thresholds(oracle, nd)
    return ro(np.stack([np.repeat(t[:, None], 256, 1), np.tile(t, (256, 1))]))


def ema_depth_frames(oracle):
    """(2, 257, 256): as ema_disp_frames for show_depthMap with IDENT; row 256 holds the anchors, and
    frame 1 is built from the thresholds of the range state that frame 0 leaves."""
    t0, t1 = depth_thresholds(oracle), depth_thresholds(oracle, range_after(ZR0))
    f = np.full((2, 257, 256), 1000.0, F32)
    f[0, :256], f[1, :256] = np.repeat(t0[:, None], 256, 1), np.tile(t1, (256, 1))
    f[:, 256, 0], f[:, 256, 1] = Z_LO, Z_HI
    return ro(f)


# ---- display: the comparisons of k_zstats and k_zrange -----------------------------------------------

def _na(v, to):
    return np.nextafter(F32(v), F32(to))


ZVALS = np.array([_na(1e4, 0), 1e4, _na(1e4, np.inf), _na(12000, 0), 12000, _na(12000, np.inf), -0.0, 0.0,
                  1e-45, 1.17549435e-38, np.nan, np.inf, -np.inf], F32)
ZPOS = [(0, 0), (0, 63), (0, 255), (0, 256), (1, WIDE - 1)]  # lane 0, lane 63, either side of a block, last pixel
ZCOMPANION = (1, 100)


def zcmp_frames():
    """(130, 2, 300, 3): frame ((v * 5 + p) * 2 + alone) holds ZVALS[v] at ZPOS[p] among NaN Z, and
    Z = 5000 at ZCOMPANION unless `alone`: the value is the frame's only candidate for the minimum
    or the maximum, or the only valid Z at all (hi == lo)."""
    rng = np.random.default_rng(12)
    n = len(ZVALS) * len(ZPOS) * 2
    x = rng.uniform(-3000, 3000, (n, 2, WIDE, 3)).astype(F32)
    x[..., 2] = np.nan
    for f in range(n):
        v, p, alone = f // 10, (f // 2) % 5, f % 2
        if not alone:
            x[(f,) + ZCOMPANION + (2,)] = 5000.0
        x[(f,) + ZPOS[p] + (2,)] = ZVALS[v]
    return ro(x)


def many_frames(F=70, H=3, W=90, seed=70):
    """(F, H, W, 3) of Z in (-3000, 12500) with the compare values sprinkled in; frames 5 and 40
    hold no valid Z, frame 20 exactly one."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3000, 12500, (F, H, W, 3)).astype(F32)
    z = x[..., 2].reshape(-1)
    at = rng.choice(len(z), 400, replace=False)
    z[at] = ZVALS[np.arange(400) % len(ZVALS)]
    x[5, :, :, 2] = np.nan
    x[40, :, :, 2] = -1.0
    x[20, :, :, 2] = 11000.0
    x[20, 1, 85, 2] = 4321.0
    return ro(x)


CLAMP_STATES = [((9999.5, 10000.0), (9999.8, 9999.9)), ((0.0, 0.5), (0.001, 0.002))]  # (state, frame Z lo / hi)


def clamp_frame(lo, hi, W=90, H=3):
    z = np.linspace(lo, hi, W * H).astype(F32).reshape(H, W)
    return ro(z)


COL0_W = (1, 63, 64, 65, 80, 81, 255, 256, 257, 300)


def col0_list(W):
    return (0, 79, 80, 81, W - 1, W, W + 5)


def coverage_frame(W, H, seed=0):
    """(H, W, 3) whose Z draws from the compare values and from (-100, 13000)."""
    rng = np.random.default_rng(seed + 1000 * W + H)
    x = rng.uniform(-100, 13000, (H, W, 3)).astype(F32)
    m = rng.random((H, W)) < 0.4
    x[..., 2][m] = ZVALS[rng.integers(0, len(ZVALS), int(m.sum()))]
    return ro(x)
