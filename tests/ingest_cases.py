"""Calibrations, sizes and map classifiers shared by the ingest edge tests (test_gpu_ingest_edges.py)
and the CPU check that the cases reach what they claim (test_ingest_cases_cpu.py).  Nothing here
needs a GPU.

The reference calibration (tests/golden/stereo.yaml) keeps every tap of its maps inside the source
but for 21 right-eye entries on the bottom row, so the border logic of the ingest kernels (partial
taps, masks, the 6-byte span's offsets at the clamped column) needs maps of its own:

  shift+ / shift-  no distortion, R = I, P = K (3 x 3) with the principal point moved by +0.5 / -0.5:
                   source coordinate (x - 0.5, y - 0.5) / (x + 0.5, y + 0.5), every fraction (16, 16),
                   so column 0 / row 0 read sx == -1 / sy == -1 (shift+) and the last column / row
                   read sx == W - 1 / sy == H - 1 (shift-).  Each output pixel is the rounded mean of
                   a 2 x 2 source neighbourhood with zeros outside: a known answer in plain numpy.
  zoom             14 distortion coefficients cut to ndist, R a rotation about z, P (3 x 4) with 0.8
                   of K's focal lengths: the output sees past all four source borders.  The eyes
                   differ in ndist and in the sign of the rotation, so a swapped eye shows.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

SIZES_ODD = [(3, 5), (37, 23), (65, 9)]            # (W, H) of one eye: BGR outputs only
SIZES_EVEN = [(2, 2), (38, 24), (64, 8), (66, 10), (130, 70)]
SIZES = SIZES_ODD + SIZES_EVEN
TINY = [(2, 2), (3, 5)]                            # too small for the class-count condition
NDIST = (0, 4, 5, 8, 12, 14)
DIST14 = np.array([-0.17, 0.03, 0.001, -0.0007, 0.002, 0.01, -0.004, 0.0008, 0.0005, -0.0003, 0.0004,
                   0.0002, 0.0, 0.0])
ANGLE = 0.03
CLASSES = ("sx==-1", "sx==W-1", "sy==-1", "sy==H-1", "outside")
MIN_CLASS = 8  # entries of every class in every zoom map (but TINY)


def camera(W, H):
    f = 0.9 * W + 20
    return np.array([[f, 0, W / 2 - 0.3], [0, 1.01 * f, H / 2 + 0.2], [0, 0, 1]])


def shift_eye(W, H, sign):
    """(K, D, R, P) of a shift calibration, sign +1 or -1."""
    K = camera(W, H)
    P = K.copy()
    P[0, 2] += 0.5 * sign
    P[1, 2] += 0.5 * sign
    return K, np.zeros(0), np.eye(3), P


def zoom_eye(W, H, ndist, angle):
    K = camera(W, H)
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    P = np.array([[0.8 * K[0, 0], 0, K[0, 2], -30.0], [0, 0.8 * K[1, 1], K[1, 2], 0], [0, 0, 1, 0]])
    return K, DIST14[:ndist].copy(), R, P


def _case(name, W, H, left, right):
    return SimpleNamespace(name=name, W=W, H=H, eyes=(left, right), id=f"{name}-{W}x{H}")


def _cases():
    out = []
    for W, H in SIZES:
        out.append(_case("shift+", W, H, shift_eye(W, H, 1), shift_eye(W, H, 1)))
        out.append(_case("shift-", W, H, shift_eye(W, H, -1), shift_eye(W, H, -1)))
        # every ndist once as the left eye and once as the right one
        for k, nd in enumerate(NDIST):
            nr = NDIST[(k + 1) % len(NDIST)]
            out.append(_case(f"zoom{nd}_{nr}", W, H, zoom_eye(W, H, nd, ANGLE), zoom_eye(W, H, nr, -ANGLE)))
    return out


CASES = _cases()
SHIFT_CASES = [c for c in CASES if c.name.startswith("shift")]
ZOOM_CASES = [c for c in CASES if c.name.startswith("zoom")]


def cases_of(W, H):
    return [c for c in CASES if (c.W, c.H) == (W, H)]


def config(case):
    """What StereoRectifier reads of a StereoConfiguration."""
    (Kl, Dl, R1, P1), (Kr, Dr, R2, P2) = case.eyes
    return SimpleNamespace(imageSize=(case.W, case.H), cameraMatrixLeft=Kl, distCoeffsLeft=Dl, R1=R1, P1=P1,
                           cameraMatrixRight=Kr, distCoeffsRight=Dr, R2=R2, P2=P2)


_MAPS = {}


def oracle_maps(oracle, case, eye):
    """The oracle's (map1, map2) of one eye, computed once (read-only)."""
    key = (case.id, eye)
    if key not in _MAPS:
        K, D, R, P = case.eyes[eye]
        m1, m2 = oracle.init_undistort_rectify_map(K, D, R, P, case.W, case.H)
        m1.setflags(write=False)
        m2.setflags(write=False)
        _MAPS[key] = (m1, m2)
    return _MAPS[key]


@lru_cache(maxsize=None)
def sbs_frames(W, H, nframes=2):
    """Side-by-side frames (F, H, 2W, 3) of random bytes (read-only)."""
    rng = np.random.default_rng(1000 * W + H)
    a = rng.integers(0, 256, (nframes, H, 2 * W, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def classify(map1, sw, sh):
    """Counts of the border classes of a map read against an sw x sh source: the entries with that
    coordinate; `outside` the entries with no tap inside; `inside` those with all four.  A key with
    "partial:" in front counts the entries of an edge class whose other coordinate leaves a tap
    inside (the pixel is a partial sum; the others are `outside` as well)."""
    sx, sy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    xin, yin = (sx >= -1) & (sx <= sw - 1), (sy >= -1) & (sy <= sh - 1)
    edge = {"sx==-1": (sx == -1, yin), "sx==W-1": (sx == sw - 1, yin), "sy==-1": (sy == -1, xin),
            "sy==H-1": (sy == sh - 1, xin)}
    n = {k: int(a.sum()) for k, (a, _) in edge.items()}
    n.update({"partial:" + k: int((a & b).sum()) for k, (a, b) in edge.items()})
    n["outside"] = int((~(xin & yin)).sum())
    n["inside"] = int(((sx >= 0) & (sx <= sw - 2) & (sy >= 0) & (sy <= sh - 2)).sum())
    return n


def shift_closed_form(src, sign):
    """The shift calibrations' answer: (a + b + c + d + 2) >> 2 over the 2 x 2 neighbourhood that
    starts at (x - 1, y - 1) (sign +1) or (x, y) (sign -1), zeros outside; src (H, W[, C]) uint8."""
    s = src.astype(np.int64)
    pad = [(1, 1), (1, 1)] + [(0, 0)] * (s.ndim - 2)
    p = np.pad(s, pad)  # p[y + 1, x + 1] = src[y, x]
    H, W = s.shape[:2]
    o = 0 if sign > 0 else 1
    q = p[o:o + H, o:o + W] + p[o:o + H, o + 1:o + 1 + W] + p[o + 1:o + 1 + H, o:o + W] + \
        p[o + 1:o + 1 + H, o + 1:o + 1 + W]
    return ((q + 2) >> 2).astype(np.uint8)


def bgr2gray_int(bgr):
    """cv::cvtColor(BGR2GRAY) on 8-bit: (1868 B + 9617 G + 4899 R + 2^13) >> 14."""
    b = bgr.astype(np.int64)
    return ((b[..., 0] * 1868 + b[..., 1] * 9617 + b[..., 2] * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def area_half_int(g):
    """cv::resize(0.5, INTER_AREA) on 8-bit, even sizes: (sum of the 2 x 2 block + 2) >> 2."""
    s = g.astype(np.int64)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
