"""The plane search without a GPU: the C structs' layout and defaults, the host-side argument guards
(every refusal comes before any device call), the Python argument checks, mix() against values
computed by hand, and the numpy restatement (tests/plane_search_ref.py) on the three-surface scene
that motivates the search: one least-squares fit of the frame lies on no surface, the search finds
all three."""
import ctypes

import numpy as np
import pytest

import plane_ref as PR
import plane_search_ref as SR
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd import _lib, pipeline
from stereo_depth_ruler_amd import synthetic as S
from stereo_depth_ruler_amd.ruler import PLANE_SEARCH_ROUND_DTYPE

Q = S.REFERENCE_Q


def test_struct_layout_and_defaults():
    P, R = _lib.PlaneSearchParams, _lib.PlaneSearchRound
    assert ctypes.sizeof(P) == 64 and ctypes.sizeof(R) == 16 and PLANE_SEARCH_ROUND_DTYPE.itemsize == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("fit", 0), ("max_planes", 32), ("hypotheses", 36), ("seed", 40), ("reserved", 44)]
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [
        ("hypothesis", 0), ("score", 4), ("voids", 8), ("stop", 12)]
    assert SR.ROUND_DTYPE == PLANE_SEARCH_ROUND_DTYPE
    assert [PLANE_SEARCH_ROUND_DTYPE.fields[n][1] for n in ("hypothesis", "score", "voids", "stop")] == [0, 4, 8, 12]
    assert (sdr.SEARCH_RAN, sdr.SEARCH_NO_HYPOTHESIS, sdr.SEARCH_LOW_SCORE, sdr.SEARCH_REFIT_DEGENERATE,
            sdr.SEARCH_FEW_INLIERS, sdr.SEARCH_NOT_RUN) == (0, 1, 2, 3, 4, 5)
    assert (SR.RAN, SR.NO_HYPOTHESIS, SR.LOW_SCORE, SR.REFIT_DEGENERATE, SR.FEW_INLIERS, SR.NOT_RUN) == (0, 1, 2, 3, 4, 5)
    L = _lib.lib()
    assert L.sdr_abi_version() == 4
    p = P(_lib.PlaneParams(9, 9, 9.0, 9.0, 9.0, (ctypes.c_int32 * 3)(9, 9, 9)), 9, 9, 9, (ctypes.c_int32 * 5)(*[9] * 5))
    L.sdr_plane_search_params_default(ctypes.byref(p))
    f = p.fit
    assert (f.iterations, f.min_inliers, f.inlier_px, f.min_disp, f.conf_min) == (3, 64, 1.0, -1.0, 0.0)
    assert list(f.reserved) == [0, 0, 0] and list(p.reserved) == [0] * 5
    assert (p.max_planes, p.hypotheses, p.seed) == (4, 256, 0)
    L.sdr_plane_search_params_default(None)


def test_host_guards_without_a_device():
    L = _lib.lib()
    Qc = (ctypes.c_double * 16)(*np.asarray(Q).reshape(16))
    ptr = ctypes.c_void_p(4096)  # never dereferenced: the guards return first
    W, H, F = 8, 6, 2

    def params(it=3, mi=16, px=1.0, mp=4, m=256):
        return _lib.PlaneSearchParams(_lib.PlaneParams(it, mi, px, -1.0, 0.0), mp, m, 0)

    def dev(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=params(), reg=ptr, out=ptr, cnt=ptr):
        return L.sdr_find_planes_device(disp, typ, stride, fs, w, h, f, None, q, ctypes.byref(par) if par else None,
                                        reg, out, cnt, None, None, None)

    def host(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=params(), reg=ptr, out=ptr, cnt=ptr):
        return L.sdr_find_planes(disp, typ, stride, fs, w, h, f, None, q, ctypes.byref(par) if par else None,
                                 reg, out, cnt, None, None)

    for fn in (dev, host):
        assert fn(disp=None) == -1 and fn(q=None) == -1 and fn(par=None) == -1
        assert fn(reg=None) == -1 and fn(out=None) == -1 and fn(cnt=None) == -1
        assert fn(w=0) == -1 and fn(h=0) == -1 and fn(f=0) == -1
        assert fn(stride=W - 1) == -1 and fn(fs=W * H - 1) == -1
        assert fn(typ=2) == -1 and fn(typ=-1) == -1
        assert fn(w=8193, stride=8193, fs=8193 * H) == -1 and fn(h=8193, fs=W * 8193) == -1
        assert fn(w=8192, stride=8192, h=4096, fs=8192 * 4096) == -1  # 2^25 pixels
        assert fn(par=params(it=9)) == -1 and fn(par=params(it=-1)) == -1 and fn(par=params(it=0)) == -1
        assert fn(par=params(mi=2)) == -1
        for px in (0.0, -1.0, float("nan"), 65.0, float("inf")):
            assert fn(par=params(px=px)) == -1, px
        assert fn(par=params(mp=0)) == -1 and fn(par=params(mp=9)) == -1 and fn(par=params(mp=-1)) == -1
        assert fn(par=params(m=0)) == -1 and fn(par=params(m=4097)) == -1 and fn(par=params(m=-5)) == -1
        assert L.sdr_last_error()


def test_python_surface_checks_arguments():
    r = sdr.Ruler(Q)
    z = np.zeros((4, 4), np.float32)
    with pytest.raises(sdr.SDRError):
        r.find_planes(np.zeros((4, 4), np.float64))
    with pytest.raises(sdr.SDRError):
        r.find_planes(z, (0, 0, 3))
    with pytest.raises(sdr.SDRError):
        r.find_planes(z, [(0, 0, 3, 3), (0, 0, 2, 2)])
    with pytest.raises(sdr.SDRError):
        r.find_planes(z, conf=np.zeros((3, 4), np.float32))
    for kw in (dict(iterations=0), dict(iterations=9), dict(max_planes=0), dict(max_planes=9), dict(hypotheses=0),
               dict(hypotheses=4097), dict(seed=-1), dict(seed=2 ** 32), dict(min_inliers=2), dict(inlier_px=0.0)):
        with pytest.raises(sdr.SDRError):
            r.find_planes(z, **kw)
    with pytest.raises(sdr.SDRError):
        r.find_planes_device(z)
    with pytest.raises(RuntimeError, match="without ruler="):
        pipeline.LiveLoop.find_planes(type("L", (), {"ruler": None})(), None, None)


def _mix_by_hand(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) % 2 ** 32
    x ^= x >> 15
    x = (x * 0x846CA68B) % 2 ** 32
    x ^= x >> 16
    return x


def test_mix_known_values():
    # computed by hand from the definition: 0 is a fixed point; 1 -> 1 * 0x7feb352d = 0x7feb352d,
    # ^ (>> 15) = 0x7feb352d ^ 0xffd6 = 0x7febcafb, * 0x846ca68b mod 2^32 = 0x6889f849,
    # ^ (>> 16) = 0x6889f849 ^ 0x6889 = 0x688990c0
    assert int(SR.mix(0)) == 0
    assert int(SR.mix(1)) == 0x688990C0
    assert int(SR.mix(0xDEADBEEF)) == 0xE628C683
    for x in (0, 1, 0xDEADBEEF, 0xFFFFFFFF, 0x9E3779B9):
        assert int(SR.mix(x)) == _mix_by_hand(x)
    xs = np.arange(1000, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(2 ** 32)
    assert SR.mix(xs).tolist() == [_mix_by_hand(int(x)) for x in xs]


def test_hypothesis_table_is_the_plane_through_its_points():
    d, _, _ = SR.three_surface_scene(33, 47)
    q, ok = PR.quantise(d[0], None, -1.0, 0.0)
    tab = SR.hypothesis_table(q, ok, 0, 97, 5)
    live = ~tab["void"]
    assert live.sum() > 50
    for j in range(3):  # every point of a hypothesis has integer residual 0, and is free
        u, v, qq = tab["pts"][live, j, 0], tab["pts"][live, j, 1], tab["pts"][live, j, 2]
        e = tab["A"][live] * u + tab["B"][live] * v + tab["C"][live] * qq - tab["D"][live]
        assert not e.any() and ok[v, u].all() and np.array_equal(q[v, u], qq)
    vv, uu = np.nonzero(ok)
    sc = SR.score_vector(tab, uu.astype(np.int64), vv.astype(np.int64), q[vv, uu], 16)
    assert (sc[live] >= 3).all() and not sc[~live].any()
    h, s, voids = SR.pick(tab, sc)
    assert s == sc.max() and h == int(np.nonzero(sc == s)[0][0]) and voids == int((~live).sum())


# The three-surface scene of the issue (320 x 240: floor 36 %, box 26 %, wall 34 % of the valid
# pixels, sigma 0.15 px, 5 % outliers, 20 % holes).  Measured with this restatement (seed 0,
# M = 256 and M = 32 alike): floor / wall / box are planes 0 / 1 / 2 with
#   |da| 1.5e-5 / 9.9e-6 / 2.8e-5,  |db| 3.9e-5 / 3.4e-5 / 2.5e-5,  |dc| 4.1e-3 / 3.4e-4 / 1.0e-3,
# label purity 0.9963 / 0.9965 / 0.9947, recall 1.000 each.  The tolerance is twice the largest
# measured error (4.12e-3, rounded up to 4.2e-3).
COEF_TOL = 2 * 4.2e-3


@pytest.fixture(scope="module")
def scene():
    d, truth, coefs = SR.three_surface_scene()
    return d, truth, coefs


def test_one_fit_fails_where_the_search_succeeds(scene):
    d, truth, coefs = scene
    H, W = truth.shape
    frame = (0, 0, 0, W - 1, H - 1)
    sizes = [int((truth == s).sum()) for s in range(3)]
    one = PR.fit_planes(d, [frame], Q, iterations=3)[0]
    print("one fit: coef", one["coef"], "inliers", one["n_inliers"], "of", one["n_valid"], "surfaces", sizes)
    assert one["flags"] == PR.OK and one["n_inliers"] < max(sizes) // 4
    for M in (256, 32):
        planes, count, rounds, labels = SR.find_planes(d, frame, Q, max_planes=4, hypotheses=M, min_inliers=1000)
        assert count == 3 and rounds["stop"].tolist()[:3] == [SR.RAN] * 3
        assert rounds["stop"][3] in (SR.LOW_SCORE, SR.NO_HYPOTHESIS)
        assert (planes["flags"][:3] == PR.OK).all() and planes["flags"][3] == PR.DEGENERATE
        matched = []
        worst = 0.0
        for s, (a, b, c) in enumerate(coefs):
            err = np.array([np.max(np.abs(p["coef"] - (a, b, c))) for p in planes[:3]])
            hits = np.nonzero(err <= COEF_TOL)[0]
            assert len(hits) == 1, (s, err)  # each surface is matched by exactly one record
            i = int(hits[0])
            matched.append(i)
            worst = max(worst, float(err[i]))
            m = labels == i
            purity, recall = float((truth[m] == s).mean()), float(m[truth == s].mean())
            print("M %d surface %d plane %d err %.3g purity %.4f recall %.4f" % (M, s, i, err[i], purity, recall))
            assert purity >= 0.99 and recall >= 0.99
            assert int(m.sum()) == planes[i]["n_inliers"]
        assert sorted(matched) == [0, 1, 2]
        assert (labels[truth < 0] == 255).mean() > 0.9 and set(np.unique(labels)) == {0, 1, 2, 255}
        # n_valid is the free pixels at the start of the round
        assert planes["n_valid"][0] == int((d[0] > -1).sum())
        assert planes["n_valid"][1] == planes["n_valid"][0] - planes["n_inliers"][0]
    # with a low stop threshold the search goes on to "find" outliers as a plane: the threshold is
    # the caller's
    _, count, rounds, _ = SR.find_planes(d, frame, Q, max_planes=4, hypotheses=256, min_inliers=64)
    assert count in (3, 4)


def test_degenerate_regions():
    d, _, _ = SR.three_surface_scene(24, 40)
    for reg in ((0, 5, 0, 5, 23), (0, 0, 7, 39, 7), (0, 3, 3, 3, 3)):
        planes, count, rounds, labels = SR.find_planes(d, reg, Q, max_planes=3, hypotheses=40, min_inliers=3)
        assert count == 0 and tuple(rounds[0]) == (-1, 0, 40, SR.NO_HYPOTHESIS)
        assert rounds["stop"].tolist()[1:] == [SR.NOT_RUN] * 2 and (labels == 255).all()
        assert (planes["flags"] == PR.DEGENERATE).all() and (planes["area"] > 0).all()
        assert np.isnan(planes["coef"]).all() and not planes["n_valid"].any()
    planes, count, rounds, labels = SR.find_planes(np.full((1, 24, 40), -1.0, np.float32), (0, 0, 0, 39, 23), Q,
                                                   hypotheses=40, min_inliers=3)
    assert count == 0 and tuple(rounds[0]) == (-1, 0, 40, SR.NO_HYPOTHESIS) and (labels == 255).all()
    planes, count, rounds, labels = SR.find_planes(d, (0, 0, 0, 40, 23), Q, hypotheses=40)
    assert count == 0 and (planes["flags"] == PR.OUT_OF_RANGE).all() and (rounds["stop"] == SR.NOT_RUN).all()
    assert not planes["area"].any()
