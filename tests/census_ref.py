"""numpy statement of the census matching cost (include/sdr/sdr.h, SDR_COST_CENSUS_9X7) and of
StereoSGBM::compute with it.  Census is this project's own definition (OpenCV has none): this
file is its pin.  Everything after the pixel cost is numpy_ref's materialised-volume formulation.
Test helper only."""
import numpy as np

from numpy_ref import SGM_3WAY, SGM_DIRS, SGM_HH, SGM_HH4, SGM_SGBM, _box_rows, _path_volume, _wta_rows, \
    sgm_effective, speckle_filter

CENSUS_OFFSETS = [(dy, dx) for dy in range(-3, 4) for dx in range(-4, 5) if (dy, dx) != (0, 0)]


def census_9x7(img):
    """uint64 [H][W]: bit k is 1 iff I(clamp(y+dy), clamp(x+dx)) < I(y, x) for the k-th offset in
    row-major order over dy = -3..3, dx = -4..4 without the centre (62 bits)."""
    I = np.asarray(img)
    assert I.ndim == 2 and I.dtype == np.uint8
    H, W = I.shape
    ys, xs = np.arange(H), np.arange(W)
    out = np.zeros((H, W), np.uint64)
    for k, (dy, dx) in enumerate(CENSUS_OFFSETS):
        nb = I[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)]
        out |= (nb < I).astype(np.uint64) << np.uint64(k)
    return out


def popcount64(v):
    v = np.ascontiguousarray(v, dtype=np.uint64)
    return np.unpackbits(v.view(np.uint8).reshape(v.shape + (8,)), axis=-1).sum(-1).astype(np.int64)


def census_pixel_cost(L, R, minD, D):
    """pc [H][W1][D] = popcount(T_left(y, x) ^ T_right(y, x - d)) on the BT path's matched columns."""
    H, W = L.shape
    maxD = minD + D
    minX1, maxX1 = max(maxD, 0), W + min(minD, 0)
    TL, TR = census_9x7(L), census_9x7(R)
    xs = np.arange(minX1, maxX1)
    out = np.zeros((H, maxX1 - minX1, D), np.int64)
    for di, d in enumerate(range(minD, maxD)):
        out[:, :, di] = popcount64(TL[:, xs] ^ TR[:, xs - d])
    return out


def census_stripes(H, bs, mode, nstripes=4):
    """(s0, end, out0) of the chains' row segments (3WAY: OpenCV's stripes; else the frame)."""
    if mode != SGM_3WAY:
        return [(0, H, 0)]
    segs = []
    sz = int(np.ceil(H / nstripes))
    overlap = (bs // 2 + 1) + int(np.ceil(0.1 * sz))
    for k in range(nstripes):
        if k * sz >= H:
            break
        segs.append((max(min(k * sz - overlap, H), 0), min((k + 1) * sz, H), k * sz))
    return segs


def census_cost_volume(L, R, minD, D, bs, P2, mode):
    """C [H][W1][D] = P2 + box of the census pixel cost (MODE_SGBM, MODE_HH, MODE_HH4 buffers)."""
    e = sgm_effective(minD, D, bs, 1, P2, 1, 0, 0, mode)
    pix = census_pixel_cost(L, R, minD, D)
    W1, s = pix.shape[1], e["SW2"]
    xi = np.clip(np.arange(W1)[:, None] + np.arange(-s, s + 1)[None, :], 0, W1 - 1)
    hs = pix[:, xi, :].sum(2)
    return e["P2"] + _box_rows(hs, 0, L.shape[0], e["SH2"], mode in (SGM_HH, SGM_HH4))


def sgm_census(L, R, minD, D, bs, P1, P2, d12, uniq, ws=0, sr=0, mode=SGM_SGBM, nstripes=4,
               uniq_rule=0, stages=3):
    """StereoSGBM::compute with the census cost, structured like numpy_ref.sgm_full_volume.
    stages: 1 median, 2 speckle (0: the LR-checked map)."""
    e = sgm_effective(minD, D, bs, P1, P2, d12, 0, uniq, mode, uniq_rule)
    H, W = L.shape
    minX1, maxX1 = max(e["maxD"], 0), W + min(minD, 0)
    W1 = maxX1 - minX1
    inv = (minD - 1) * 16
    if W1 <= 0:
        return np.full((H, W), inv, np.int16)
    pix = census_pixel_cost(L, R, minD, D)
    s = e["SW2"]
    xi = np.clip(np.arange(W1)[:, None] + np.arange(-s, s + 1)[None, :], 0, W1 - 1)
    hs = pix[:, xi, :].sum(2)
    raw = np.full((H, W), inv, np.int64)
    for s0, end, out0 in census_stripes(H, bs, mode, nstripes):
        C = e["P2"] + _box_rows(hs, s0, end, e["SH2"], mode in (SGM_HH, SGM_HH4))
        assert C.max() <= 32767, "outside the int16 cost domain"
        Ssum = np.zeros_like(C)
        for dx, dy in SGM_DIRS[mode]:
            Lr = _path_volume(C, dx, dy, e["P1"], e["P2"])
            assert Lr.min() >= 0 and Lr.max() <= 32767
            Ssum += Lr
        Ssum = np.minimum(Ssum, 32767)
        raw[out0:end] = _wta_rows(Ssum[out0 - s0:], e, W, minX1)
    out = raw.astype(np.int16)
    if stages & 1:
        from scipy.ndimage import median_filter
        out = median_filter(out, size=3, mode="nearest")
    if (stages & 2) and ws > 0:
        out = speckle_filter(out, inv, ws, 16 * sr)
    return out
